// Device state of the keyframe point-set calls (include/eds_hip_kfpoints.h, eds_kfpoints.hip).  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct eds_trk;

#define EDS_KFP_PAR 24              // doubles of one alignment's projection block: R (9), t (3), K_src (4), K_dst (4), dst_W, dst_H, seeded, -
#define EDS_KFP_BATCH 64            // alignments per launch of k_kfp_project (its pinned outputs: 28 bytes per point and alignment)

// Allocated at the first eds_kfp_* call that needs them: a handle that never calls them keeps its memory and launches.
struct EdsKfpBuffers {
    double* range = nullptr;            // [B][Np] max - min of every original point's window
    unsigned char* erase = nullptr;     // [B][Np] the points to erase
    double* coord = nullptr;            // [B][Np][2] scratch of the compaction (getCoord's coordinates, unused)
    int* kept = nullptr;                // [B][Np] kept indices of the compaction
    // the projection's pinned, device-mapped block of `cap` alignments: par | n | xy | idp | src (h_: host view, d_: device view)
    char* h_block = nullptr;
    int cap = 0;
    double *h_par = nullptr, *d_par = nullptr;      // [cap][EDS_KFP_PAR]
    int *h_n = nullptr, *d_n = nullptr;             // [cap]
    double *h_xy = nullptr, *d_xy = nullptr;        // [cap][Np][2]
    double *h_idp = nullptr, *d_idp = nullptr;      // [cap][Np]
    int *h_src = nullptr, *d_src = nullptr;         // [cap][Np]
};

void eds_kfp_free(EdsKfpBuffers* kb);
