// What eds_pixsel.hip and eds_immature.hip share: the definition of the opaque eds_sel of include/eds_hip_select.h
// (eds_imm_create_points_selected reads its selection list in device memory).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "eds_device_owner.hpp"
#include "eds_pixsel.hpp"

struct eds_sel {
    edscapi::DeviceOwner own;
    int H = 0, W = 0;
    edspix::Geo g;
    edspix::Params prm;
    int potential = 3;
    bool table_set = false, image_set = false, hist_valid = false, sel_valid = false;
    int max_slots = 0, n_blocks256 = 0;
    int n_sel = 0, ambiguous = 0, n2_certain = 0;      // of the selection that holds
    edspix::Px* lv[edspix::LEVELS] = {nullptr, nullptr, nullptr};
    float *in_img = nullptr, *B = nullptr;             // [H * W], [256]
    float *ths = nullptr, *ths_s = nullptr;            // [w32 * h32]
    uint8_t *map = nullptr, *table = nullptr;          // [H * W]
    uint32_t* mask = nullptr;                          // [max_slots] the direction mask of every pot cell, in visiting order
    int32_t* n2_start = nullptr;                       // [max_slots] n2 when the cell is entered
    uint8_t* cell_sel = nullptr;                       // [max_slots] the cell selects at level 0
    int32_t* counts = nullptr;                         // n2, n3, n4, ambiguous cells, n2 of the certain cells, list length
    int32_t* block_cnt = nullptr;                      // [2][n_blocks256] non-zero map pixels per 256
    int32_t* uv = nullptr;                             // [H * W][2] the selection list
    float* type = nullptr;                             // [H * W]
};
