// Device state of the epiline tracker (include/eds_hip_epiline.h, eds_epiline.hip).  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct eds_trk;

// Allocated at the first eds_epi_* call of a handle: a handle that never calls them keeps its memory and launches.
struct EdsEpiBuffers {
    double* ef = nullptr;               // [2][B][Np] fp64 SoA: the ef plane, index-aligned with the slot's points (Slot::epi_valid)
    double* kpix = nullptr;             // [B][Np][2] keyframe pixels as the slot holds them (cell + fp32 fraction)
    double* mval = nullptr;             // [B][Np] getSparseModel's normalised values
    uint64_t* keys_tmp = nullptr;       // [B][Np] splat keys (k_klt_bin)
    uint64_t* keys = nullptr;
    int* row_start = nullptr;           // [B][H + 2], biased by one: entry y0 + 1 is the first key of splat row y0 = -1 .. H - 1
    double* model = nullptr;            // [B][H][W] the blurred model image
    double* par = nullptr;              // [B][EDS_EPI_PAR] per-alignment parameters (device) ...
    double* h_par = nullptr;            // ... and their pinned staging
    uint64_t* best = nullptr;           // [B][Np][2] (ssd, ncc) arg-extremum keys
    double* ef_tmp = nullptr;           // [B][Np][2] p_ssd of every original point
    int32_t* loc = nullptr;             // [B][Np][4] p_ssd, p_ncc of every original point
    double* score = nullptr;            // [B][Np][2] the two winning scores
    unsigned char* erase = nullptr;     // [B][Np] the cull
    double* coord = nullptr;            // [B][Np][2] scratch of the compaction (getCoord's coordinates, unused)
    int* kept = nullptr;                // [B][Np] kept indices of the compaction
    double* ef_aos = nullptr;           // [B][Np][2] the ef plane as eds_depth_update's EF_COORD input
    // per-radius work buffers of one chunk of alignments, grown on demand
    float* pad = nullptr; size_t pad_cap = 0;           // [chunk][(H + 2r) (W + 2r)] padded search image
    double* rowsq = nullptr; size_t rowsq_cap = 0;      // [chunk][(H + 2r) W] row sums of squares
    float2* energy = nullptr; size_t energy_cap = 0;    // [chunk][H W] (E, sqrt E) as fp32
    int2* taps = nullptr; size_t taps_cap = 0;          // [chunk][Np][(2r+1)^2] non-zero template taps (LDS offset, fp32 value)
    float4* tmeta = nullptr; size_t tmeta_cap = 0;      // [chunk][Np] (tap count, S, sqrt S, -)
};

