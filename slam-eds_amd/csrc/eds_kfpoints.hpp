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

// eds_kfp_project_depth_map's checks of T7 (count x 7) and K_dst (count x 4), either may be NULL
int eds_kfp_check_transforms(int count, const double* T7, const double* K_dst);
// fills the projection blocks of slots first .. first + cn - 1 (h_par / d_par: the two views of mapped pinned memory, EDS_KFP_PAR doubles
// per slot) and queues k_kfp_project on the handle's stream: slot first + b writes d_n[b] and, at b * Np, d_xy, d_idp and d_src
int eds_kfp_project_queue(eds_trk* h, int first, int cn, const double* T7, const double* K_dst, double dW, double dH, double* h_par,
                          const double* d_par, int* d_n, double* d_xy, double* d_idp, int* d_src);
