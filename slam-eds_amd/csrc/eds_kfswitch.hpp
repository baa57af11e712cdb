// Device state of the batched keyframe switch (include/eds_hip_kfswitch.h, eds_kfswitch.hip).  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#define EDS_KFS_CHUNK 16            // slots queued between two waits (VGA: 92 bytes per pixel and slot of work planes)

// Allocated at the first eds_kfs_* call that needs them: a handle that never calls them keeps its memory and launches.
struct EdsKfsBuffers {
    bool lds_set = false;               // k_kd_build may ask for its dynamic LDS
    // maps of a chunk, `map_stride` points per slot: as given / projected, then in tree order
    size_t map_stride = 0;
    double *d_mxy = nullptr, *d_midp = nullptr, *d_txy = nullptr, *d_tidp = nullptr;
    int *d_msrc = nullptr, *d_perm = nullptr;
    int *d_mn = nullptr, *d_flag = nullptr, *d_summary = nullptr;       // [CHUNK], [CHUNK], [CHUNK][4]
    double *d_K = nullptr;                                              // [CHUNK][4]
    // pinned: h_mn [CHUNK] | h_summary [CHUNK][4] | h_K [CHUNK][4] | par [CHUNK][EDS_KFP_PAR] (mapped: d_par is its device view)
    char* h_block = nullptr;
    int *h_mn = nullptr, *h_summary = nullptr;
    double *h_K = nullptr, *h_par = nullptr, *d_par = nullptr;
    // image work planes of a chunk, H * W elements per slot (what EdsKeyframeBuffers holds for one slot)
    void* d_raw = nullptr;
    double *d_log = nullptr, *d_gx = nullptr, *d_gy = nullptr, *d_mag = nullptr, *d_partial = nullptr;
    int *d_cand = nullptr, *d_cnt = nullptr, *d_off = nullptr;
    double *d_coord = nullptr, *d_grad = nullptr, *d_idp = nullptr, *d_w = nullptr;
    double* h_out = nullptr;            // pinned [CHUNK][6][out_n]: coord (2), grad (2), idp, w of every slot's first out_n points
    size_t out_n = 0;
};

