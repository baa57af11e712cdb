// What eds_immature.hip, eds_activate.hip and eds_immdepth.hip share: the definition of the opaque eds_imm of include/eds_hip_immature.h
// and the state include/eds_hip_activate.h and include/eds_hip_immdepth.h keep beside it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "eds_activate.hpp"
#include "eds_device_owner.hpp"
#include "eds_immature.hpp"
#include "eds_map_internal.hpp"

// include/eds_hip_activate.h's part of an eds_imm: the first eds_act_* call that needs it allocates it through the eds_imm's owner, which
// frees the device memory with the handle; act_release deletes the struct
struct eds_act_state {
    edsact::Params prm;
    edsact::Calib cal;
    bool calib_set = false, map_valid = false, sel_valid = false, fit_valid = false;
    int sel_hosts = 0;                                 // n_hosts of the selection that holds
    int stride = 0;                                    // residual columns per point: min(max_hosts, edsact::MAX_FRAMES)
    uint8_t* map = nullptr;                            // [h1 * w1]
    uint32_t* mark = nullptr;                          // [h1 * w1] the candidate loop's frontier tags
    int32_t* fate = nullptr;                           // [max_hosts][max_points]
    float* fit = nullptr;                              // [max_hosts][max_points][4] idepth, E, Hdd, bd
    int32_t* res_state = nullptr;                      // [max_hosts][max_points][stride]
    float* res_energy = nullptr;
    float *krki = nullptr, *kt = nullptr, *pre = nullptr;   // [max_hosts][9], [max_hosts][3], [stride * stride][14]
    int32_t *n = nullptr, *counts = nullptr;           // [max_hosts] points per host; [NUM_FATES]
    uint8_t* flagged = nullptr;                        // [max_hosts]
    float* active = nullptr;                           // staging for active points handed over in host memory
    int32_t* active_host = nullptr;
    int active_cap = 0;
};

struct eds_imd_state;                                  // include/eds_hip_immdepth.h's part, defined in eds_immdepth.hip

struct eds_imm {
    edscapi::DeviceOwner own;
    int H = 0, W = 0, max_hosts = 0, max_points = 0, max_targets = 0;
    edsimm::Params prm;
    float *host_c = nullptr, *target_c = nullptr;      // [frames][H][W]
    edsimm::Grad *host_g = nullptr, *target_g = nullptr;
    edsimm::Point* points = nullptr;                   // [max_hosts][max_points]
    edsimm::Pre* pre = nullptr;                        // [max_hosts]
    int32_t* summary = nullptr;                        // [max_hosts][NUM_STATUS]
    double* in_distance = nullptr;                     // eds_imm_create_points' inputs, [max_points] each
    int32_t* in_uv = nullptr;
    float *in_type = nullptr, *in_idepth = nullptr;
    uint8_t* in_alive = nullptr;
    std::vector<int> n;
    std::vector<uint8_t> host_set, target_set;
    eds_act_state* act = nullptr;
    eds_map_state* map = nullptr;                      // include/eds_hip_map.h's scratch, allocated by the first eds_map_immature_cloud
    eds_imd_state* imd = nullptr;                      // the depth map, its tree and the nearest points, allocated by the first eds_imd_* call
};

namespace edsimm_internal {
// eds_activate.hip
void act_release(eds_imm* h);
void act_invalidate(eds_imm* h);                       // a host's image or points were replaced: map, selection and fit no longer hold
// eds_immdepth.hip
void imd_release(eds_imm* h);                          // after the owner closed: deletes the struct and its events
}  // namespace edsimm_internal
