// What eds_init.hip and eds_inisetup.hip share: the definition of the opaque eds_ini of include/eds_hip_init.h, the state
// include/eds_hip_inisetup.h keeps beside it, and the one step of eds_init.hip the set-up calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "eds_device_owner.hpp"
#include "eds_init.hpp"

struct eds_ini {
    edscapi::DeviceOwner own;
    int cap = 0;
    edsct::Geo geo;
    edsini::Params prm;
    bool calib_set = false, first_set = false, new_set = false;
    bool points_set[edsini::MAX_LEVELS] = {false, false, false, false, false}, tables_set[edsini::MAX_LEVELS] = {false, false, false, false, false};
    int32_t n[edsini::MAX_LEVELS] = {0, 0, 0, 0, 0}, nd[edsini::MAX_LEVELS] = {0, 0, 0, 0, 0};
    float exposure_first = 1.0f;
    edsini::Carry carry;                                   // the host's copy of what the device hands from frame to frame
    edsdso::Px *first_px = nullptr, *new_px = nullptr;      // [geo.total]
    float *in_img = nullptr, *in_status = nullptr;         // [H * W]
    edsini::Pnt* pts = nullptr;                            // [levels][cap]
    int32_t *sched = nullptr, *parent = nullptr, *doff = nullptr, *coff = nullptr, *child = nullptr;
    float *jb = nullptr, *iR_old = nullptr;
    int32_t *good_old = nullptr, *d_count = nullptr;
    edsini::Carry* d_carry = nullptr;
    edsini::Result* d_out = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;               // around k_ini_track, for eds_ini_get_kernel_ms
    float kernel_ms = -1.0f;
    long n_launches = 0, n_waits = 0;                      // counted where a file launches and waits: INI_LAUNCH, ini_wait, ini_read_back

    // include/eds_hip_inisetup.h's part.  The first call that needs device memory allocates it through `own`, which frees it with the
    // handle.  sparsity is the reference's global sparsityFactor (src/utils/settings.cpp:212).
    int32_t sparsity = 5;
    bool status_set[edsini::MAX_LEVELS] = {false, false, false, false, false};    // the level's map is of the first frame that holds
    bool nn_made[edsini::MAX_LEVELS] = {false, false, false, false, false};       // nn holds the tables the level's schedule was derived from
    uint8_t* status = nullptr;                             // [geo.total] one byte per pixel, the levels at geo.l[].off
    float2* uv = nullptr;                                  // [levels][cap] the points' (u, v), packed for the search
    edsnn::Node* tree_nodes = nullptr;                     // [2][2 cap] the k-d tree of the level eds_ini_make_neighbours works on, and of the level above
    int32_t* tree_vind = nullptr;                          // [2][cap] their permuted point indices
    int32_t* nn = nullptr;                                 // [levels][cap][11] ten neighbours and the parent
    float nn_kernel_ms = -1.0f;
};

namespace edsini_internal {
// eds_init.hip: one level's points from a map of bytes in device memory (w x h of the level, dense; non-zero: selected, the value is
// my_type) with everything eds_ini_set_points does after its upload
int points_from_bytes(eds_ini* h, int lvl, const uint8_t* map, int32_t* n_out);
}  // namespace edsini_internal
