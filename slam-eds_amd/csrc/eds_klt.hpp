// Device state of the KLT point trackers (include/eds_hip_klt.h, eds_klt.hip).  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct eds_trk;

// Allocated at the first eds_klt_track_points* of a handle: a handle that never calls KLT keeps its memory and launches.
struct EdsKltBuffers {
    double* tracks = nullptr;       // [2][B][Np] fp64 SoA: kf->tracks (x plane, then y plane)
    double* flow = nullptr;         // [2][B][Np] fp64 SoA: kf->flow
    double* coord = nullptr;        // [B][Np][2] the warped coordinates getCoord(true) left for the window kernel
    int* kept = nullptr;            // [B][Np] the kept indices of that getCoord
    uint64_t* keys_tmp = nullptr;   // [B][Np] splat_key(y0, x0, i) (eds_splat.hpp) in arrival order (binning scratch)
    uint64_t* keys = nullptr;       // [B][Np] the same keys sorted by (y0, x0, i)
    int* row_start = nullptr;       // [B][H + 2] first key of splat row y0 = 0 .. H, then the number of binned points
};

// device outputs of getCoord for the KLT, indexed by slot, in HBM (eds_points.hip writes them instead of the pinned block).
// erase ([B][Np], indexed by slot, or null): the points to erase are those flagged non-zero instead of those that left the frame,
// and the KLT's tracks plane is compacted like the flow instead of being rewritten (the epiline cull, eds_epiline.hip)
struct EdsPointsDev {
    double* coord;
    int* kept;
    const unsigned char* erase = nullptr;
};

// a new keyframe: zero the slot's tracks and flow (KeyFrame::create, KeyFrame.cpp:447-448), on the handle's stream
void eds_klt_reset_slot(eds_trk* h, int slot);
// k_klt_bin for slots first .. first + count - 1 over the pixel coordinates `coord` ([B][Np][2], indexed by slot): keys and row starts
// as the KLT's window kernel reads them (bias 0: the points getCoord(true) keeps).  bias 1 is the epiline model image's
// (eds_epiline.hip): every point with -1 < x < W, -1 < y < H, keyed and binned by (y0 + 1, x0 + 1)
int eds_klt_bin_launch(eds_trk* h, int first, int count, const double* coord, uint64_t* keys_tmp, uint64_t* keys, int* row_start, int bias);
