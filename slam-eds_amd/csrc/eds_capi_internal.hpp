// Internals shared by the three translation units of the C ABI (include/eds_hip.h):
//   eds_capi.hip          handle lifecycle, configuration, knobs, states, sync / info, the rows around the path (points, keyframes)
//   eds_capi_inputs.hip   what goes INTO a slot: keyframe points, inverse depths, event frames (host buffers or events), shared frames
//   eds_capi_solve.hip    the passes and solves: eval, the host-driven loop (EDS_EXEC_HOST), optimize, residuals, loss scale, bench hooks
// Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>

#include "../../include/eds_hip.h"
#include "eds_device_owner.hpp"                       // fail, EDS_HIP_TRY, DevAlloc
#include "eds_fused.hpp"
#include "eds_handle.hpp"
#include "eds_kernels.hpp"
#include "eds_math.hpp"
#include "eds_solver.hpp"

namespace edscapi {

// eds_capi.hip
int effective_blocks(const eds_trk* h);
int level_iters(const eds_trk* h, int level);
int check_slot(const eds_trk* h, int slot);
int check_range(const eds_trk* h, int first, int count);
void fill_static(const eds_trk* h, int slot);
void fill_pose(eds_trk* h, int slot, const double* p, const double* q, const double* v);
int upload_pose(eds_trk* h, int first, int count);
int max_points(const eds_trk* h, int first, int count);       // the largest N of the slots first .. first + count - 1
// After check_range / check_slot and the call's argument checks: "no batch in flight" (EDS_ERR_STATE), then per slot, in this order, what
// `need` asks for: a keyframe with N >= 1, an event frame, initialised depth seeds (EDS_ERR_STATE with the condition's message)
enum { EDS_NEED_KF = 1, EDS_NEED_FRAME = 2, EDS_NEED_SEEDS = 4 };
int check_idle_slots(const eds_trk* h, int first, int count, int need);
// rows first .. first + count - 1 of an [2][B][Np] fp64 plane (x plane, then y plane) into the caller's interleaved dst[count][stride][2],
// the first slots[first + b].N points of row b; waits for the stream
int read_xy_planes(eds_trk* h, const double* plane, int first, int count, int stride, double* dst);
int workgroup_lds_limit(const eds_trk* h, size_t* bytes);     // selects the handle's device; the LDS one workgroup may ask for
bool row_bins_fit(const eds_trk* h, size_t limit);            // k_klt_bin's two [H + 2] int arrays fit `limit`, H and W fit a key's 16 bits
// eds_trk_update_points_batch after its argument checks; dev: see eds_points_update_batch
int update_points_range(eds_trk* h, int first, int count, int delete_out_points, int stride, double* coord_xy, double* tracks_xy,
                        int32_t* kept_index, int* n_kept, double* mean_sq_flow, const EdsPointsDev* dev = nullptr);
// eds_capi_inputs.hip
int refresh_gram(eds_trk* h, int slot, bool wait = true);
int unshare_frames(eds_trk* h, int first, int count);       // slots about to receive a frame of their own stop sampling somebody else's
// eds_capi_solve.hip
int solve_host(eds_trk* h, int level, int first, int count);
int materialise_residuals(eds_trk* h, int slot);

}  // namespace edscapi
