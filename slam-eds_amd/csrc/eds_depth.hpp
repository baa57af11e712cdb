// Device state of the inverse-depth filter (include/eds_hip_depth.h, eds_depth.hip).  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#define EDS_DP_STRIDE 48            // doubles of one alignment's parameter block (eds_depth.hip: EDS_DP_*)

struct eds_trk;

// Allocated at the first eds_depth_init of a handle: a handle that never uses the filter keeps its memory and launches.
struct EdsDepthBuffers {
    double* seeds = nullptr;        // [4][B][Np] fp64 SoA: mu, sigma2, a, b — a wavefront's loads of one plane coalesce
    double* d_par = nullptr;        // [B][EDS_DP_STRIDE] per-alignment parameters of the last launch (copied from h_par)
    double* h_par = nullptr;        // pinned
    int* d_sum = nullptr;           // [B][6] summary counters (eds_depth_summary)
    int* h_sum = nullptr;           // pinned
    double* d_stats = nullptr;      // [B][4] meanIDepth / medianIDepth
    double* h_stats = nullptr;      // pinned
    double* d_in = nullptr;         // [2][B][Np][2] host inputs of an update (xy, kf_xy) or of init / set; allocated at first need
};

// getCoord's compaction of slots first .. first + count - 1 has just been launched with its kept indices in `kept` ([count][Np],
// device view): gather the seeds of those slots the same way, on the same stream (eds_points.hip)
void eds_depth_compact(eds_trk* h, int first, int count, const int* kept);
struct eds_depth_summary;
// eds_depth_update's body.  dev_ef (or null): EDS_DEPTH_EF_COORD's coordinates already in HBM, [count][Np][2] (b relative to
// first) — the epiline's ef plane (eds_epiline.hip); xy is then not read
int eds_depth_update_impl(eds_trk* h, int first, int count, int coords, const double* xy, const double* kf_xy, int stride,
                          const double* T_kf_ef, int filter, eds_depth_summary* out, const double* dev_ef);
