"""ctypes binding of the C-ABI library ``csrc/libeds_hip.so`` (header: ``include/eds_hip.h``).

This is plumbing only: every number is produced by the HIP kernels behind the C ABI.
There is no CPU fallback — if the library is missing or no GPU is visible the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import NamedTuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
LIB_PATH = os.environ.get("EDS_HIP_LIB") or os.path.join(CSRC, "libeds_hip.so")   # env override: diagnostic builds only

# enums of include/eds_hip.h
EDS_OK = 0
ERR_INVALID, ERR_HIP, ERR_NOT_USABLE, ERR_STATE, ERR_NO_DEVICE = -1, -2, -3, -4, -5
SAMPLE_BICUBIC, SAMPLE_BILINEAR = 0, 1
SOLVER_GN6, SOLVER_LM6, SOLVER_REF12 = 0, 1, 2
EXEC_HOST, EXEC_DEVICE = 0, 1
LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY = 0, 1, 2
LP_CONSTANT, LP_MAD, LP_STD = 0, 1, 2
KF_MAX, KF_MEDIAN = 0, 1
IMG_U8, IMG_F32, IMG_F64 = 0, 1, 2
MAX_LEVELS = 8

# every symbol include/eds_hip.h declares (tests check the .so exports all of them)
EXPORTS = (
    "eds_abi_version", "eds_device_count", "eds_last_error", "eds_trk_cfg_default", "eds_trk_cfg_size",
    "eds_trk_info_size",
    "eds_trk_create", "eds_trk_destroy", "eds_trk_set_config", "eds_trk_get_config",
    "eds_trk_set_keyframe", "eds_trk_set_idepth", "eds_trk_set_idepth_strided", "eds_trk_set_event_frame", "eds_trk_set_event_frame_f32", "eds_trk_set_event_frames", "eds_trk_set_event_frames_f32",
    "eds_trk_set_undistort_map", "eds_trk_set_undistort_map_sized", "eds_trk_build_event_frame", "eds_trk_build_event_frames", "eds_trk_build_event_frame_batch", "eds_trk_build_event_frames_aos", "eds_trk_build_event_frames_aos_timed", "eds_event_times_aos",
    "eds_trk_get_event_frame", "eds_trk_share_event_frame",
    "eds_trk_set_state", "eds_trk_get_state", "eds_trk_set_states", "eds_trk_get_states", "eds_trk_get_results",
    "eds_trk_eval", "eds_trk_optimize", "eds_trk_optimize_batch", "eds_trk_optimize_batch_wait",
    "eds_trk_sync", "eds_trk_get_info", "eds_trk_get_trace", "eds_trk_get_residuals", "eds_trk_loss_param", "eds_trk_residuals_and_loss",
    "eds_trk_loss_param_batch", "eds_trk_update_points", "eds_trk_update_points_batch",
    "eds_kf_select_default", "eds_trk_build_keyframe", "eds_trk_build_keyframe_image", "eds_trk_get_keyframe_points",
    "eds_trk_timer_start", "eds_trk_timer_stop", "eds_trk_bench_eval", "eds_trk_bench_live", "eds_trk_bench_batch", "eds_trk_last_launch", "eds_trk_prepare_frames",
    "eds_trk_set_knob", "eds_trk_get_strips_info", "eds_trk_bench_kernel_cold", "eds_trk_hbm_probe", "eds_trk_kernel_instances",
    "eds_pyr_create", "eds_pyr_destroy", "eds_pyr_set_config", "eds_pyr_level_intrinsics", "eds_pyr_set_keyframe",
    "eds_pyr_set_event_frame", "eds_pyr_build_event_frame", "eds_pyr_level_size", "eds_pyr_get_level_frame", "eds_pyr_optimize",
    "eds_pyr_get_residuals", "eds_pyr_create_batch", "eds_pyr_set_keyframe_slot", "eds_pyr_set_event_frame_slot", "eds_pyr_optimize_batch",
)

# every symbol include/eds_hip_depth.h declares: the inverse-depth filter (its own header and ABI version; EXPORTS stays eds_hip.h's)
DEPTH_EXPORTS = (
    "eds_depth_abi_version", "eds_depth_params_default", "eds_depth_init", "eds_depth_update", "eds_depth_get", "eds_depth_set",
    "eds_depth_get_idepth", "eds_depth_stats",
)
# enums of include/eds_hip_depth.h
DEPTH_INIT_CONSTANT, DEPTH_INIT_HOST, DEPTH_INIT_PLANE = 0, 1, 2
DEPTH_TRACKS, DEPTH_EF_COORD, DEPTH_REPROJECT, DEPTH_DEVICE_TRACKS = 0, 1, 2, 3
DEPTH_VOGIATZIS, DEPTH_GAUSS = 0, 1

# every symbol include/eds_hip_klt.h declares: the KLT point trackers (their own header and ABI version)
KLT_EXPORTS = ("eds_klt_abi_version", "eds_klt_track_points", "eds_klt_track_points_pyr", "eds_klt_get")

# every symbol include/eds_hip_epiline.h declares: the epiline tracker (its own header and ABI version)
EPI_EXPORTS = ("eds_epi_abi_version", "eds_epi_track_points", "eds_epi_get", "eds_epi_get_model", "eds_epi_depth_update")
# enum eds_epi_border: cv::BORDER_* (BORDER_DEFAULT = REFLECT_101)
EPI_BORDER_CONSTANT, EPI_BORDER_REPLICATE, EPI_BORDER_REFLECT, EPI_BORDER_REFLECT_101 = 0, 1, 2, 4

# every symbol include/eds_hip_kfpoints.h declares: refine / clean / erase a keyframe's points, its counts, the next keyframe's depth map
KFP_EXPORTS = ("eds_kfp_abi_version", "eds_kfp_refine_points", "eds_kfp_clean_points", "eds_kfp_erase_points", "eds_kfp_counts",
               "eds_kfp_project_depth_map")

# every symbol include/eds_hip_kfswitch.h declares: the depth k-d tree built on the device, KeyFrame::create for a range of slots
KFS_EXPORTS = ("eds_kfs_abi_version", "eds_kfs_tree_capacity", "eds_kfs_chunk_size", "eds_kfs_build_tree", "eds_kfs_build_keyframes",
               "eds_kfs_build_keyframes_dev")
KFS_DEPTH_NONE, KFS_DEPTH_HOST, KFS_DEPTH_DEVICE, KFS_DEPTH_SLOTS = 0, 1, 2, 3      # enum eds_kfs_depth_source

# every symbol include/eds_hip_immature.h declares: DSO's immature points traced along epipolar lines (bound in immature.py)
IMM_EXPORTS = ("eds_imm_abi_version", "eds_imm_params_default", "eds_imm_create", "eds_imm_destroy", "eds_imm_set_params", "eds_imm_get_params",
               "eds_imm_set_host_images", "eds_imm_set_target_images", "eds_imm_create_points", "eds_imm_num_points", "eds_imm_trace",
               "eds_imm_get", "eds_imm_get_points", "eds_imm_get_image", "eds_imm_create_points_selected")

# every symbol include/eds_hip_coarse.h declares: DSO's coarse image tracker (bound in coarse.py)
CT_EXPORTS = ("eds_ct_abi_version", "eds_ct_params_default", "eds_ct_create", "eds_ct_destroy", "eds_ct_set_params", "eds_ct_get_params",
              "eds_ct_set_calib", "eds_ct_get_k", "eds_ct_set_ref", "eds_ct_set_new", "eds_ct_track", "eds_ct_calc_res", "eds_ct_get_level")

# every symbol include/eds_hip_window.h declares: the window optimiser's linearize, applyRes and per-point sums (bound in window.py)
WIN_EXPORTS = ("eds_win_abi_version", "eds_win_params_default", "eds_win_create", "eds_win_destroy", "eds_win_set_params", "eds_win_get_params",
               "eds_win_set_calib", "eds_win_set_frames", "eds_win_get_frame", "eds_win_set_points", "eds_win_set_idepths", "eds_win_set_residuals",
               "eds_win_linearize", "eds_win_apply", "eds_win_point_hessians", "eds_win_accumulate", "eds_win_acc_size", "eds_win_get_residuals", "eds_win_get_points")

# every symbol include/eds_hip_winsolve.h declares: the window's solve, point step, energies and point marginalisation (bound in winsolve.py)
WSV_EXPORTS = ("eds_wsv_abi_version", "eds_wsv_set_state", "eds_wsv_fix_linearization", "eds_wsv_solve", "eds_wsv_backup_idepths",
               "eds_wsv_step_idepths", "eds_wsv_get_steps", "eds_wsv_l_energy", "eds_wsv_m_energy", "eds_wsv_marginalize_points", "eds_wsv_get")

# every symbol include/eds_hip_winedit.h declares: the window's tables edited on the device (bound in winedit.py)
WED_EXPORTS = ("eds_wed_abi_version", "eds_wed_remove_residuals", "eds_wed_remove_points", "eds_wed_marginalize_frame", "eds_wed_insert_activated", "eds_wed_set_state",
               "eds_wed_counts", "eds_wed_get")

# every symbol include/eds_hip_winflag.h declares: each point's residual history on the device (bound in winflag.py)
WFL_EXPORTS = ("eds_wfl_abi_version", "eds_wfl_set_history", "eds_wfl_get_history", "eds_wfl_insert_frame_residuals", "eds_wfl_apply_fixed",
               "eds_wfl_params_default", "eds_wfl_flag_points", "eds_wfl_get_fates", "eds_wfl_marginalize_flagged", "eds_wfl_remove_flagged")

# every symbol include/eds_hip_activate.h declares: the distance map, the candidate rule and the idepth fit over an eds_imm (bound in activate.py)
ACT_EXPORTS = ("eds_act_abi_version", "eds_act_params_default", "eds_act_set_params", "eds_act_get_params", "eds_act_set_calib",
               "eds_act_make_distance_map", "eds_act_get_distance_map", "eds_act_select", "eds_act_optimize", "eds_act_get", "eds_act_get_activated")

# every symbol include/eds_hip_select.h declares: DSO's pixel selector over its own eds_sel (bound in select.py)
SEL_EXPORTS = ("eds_sel_abi_version", "eds_sel_params_default", "eds_sel_create", "eds_sel_destroy", "eds_sel_set_params", "eds_sel_get_params",
               "eds_sel_set_random_pattern", "eds_sel_fill_reference_pattern", "eds_sel_set_potential", "eds_sel_get_potential", "eds_sel_set_image",
               "eds_sel_make_maps", "eds_sel_get_map", "eds_sel_get_selection", "eds_sel_get_level", "eds_sel_get_thresholds", "eds_sel_get_scan_info")

# every symbol include/eds_hip_init.h declares: DSO's two-frame initialiser over its own eds_ini (bound in init.py)
INI_EXPORTS = ("eds_ini_abi_version", "eds_ini_params_default", "eds_ini_create", "eds_ini_destroy", "eds_ini_set_params", "eds_ini_get_params",
               "eds_ini_set_calib", "eds_ini_set_first", "eds_ini_set_pose", "eds_ini_set_points", "eds_ini_set_points_selected", "eds_ini_set_neighbours",
               "eds_ini_make_nn", "eds_ini_get_schedule_depth", "eds_ini_track_frame", "eds_ini_get_kernel_ms", "eds_ini_get_points", "eds_ini_get_jb", "eds_ini_get_level")

# every symbol include/eds_hip_inisetup.h declares: the rest of setFirst over the same eds_ini (bound in init.py)
INISETUP_EXPORTS = ("eds_ini_setup_abi_version", "eds_ini_get_sparsity", "eds_ini_set_sparsity", "eds_ini_make_pixel_status",
                    "eds_ini_get_pixel_status", "eds_ini_set_points_status", "eds_ini_make_neighbours", "eds_ini_get_neighbours",
                    "eds_ini_get_neighbours_kernel_ms", "eds_ini_setup_levels")

# every symbol include/eds_hip_undistort.h declares: dso::Undistort with its PhotometricUndistorter over its own eds_und (bound in undistort.py)
UND_EXPORTS = ("eds_und_abi_version", "eds_und_settings_default", "eds_und_create", "eds_und_destroy", "eds_und_get_K", "eds_und_get_map",
               "eds_und_is_passthrough", "eds_und_set_map", "eds_und_set_photometric", "eds_und_set_settings", "eds_und_get_settings",
               "eds_und_set_form", "eds_und_get_form", "eds_und_process", "eds_und_image", "eds_und_get_image")

# every symbol include/eds_hip_map.h declares: the window's, the immature points' and a slot's point cloud, and the next keyframe's depth maps (bound in map.py)
MAP_EXPORTS = ("eds_map_abi_version", "eds_map_window_cloud", "eds_map_window_depth_maps", "eds_map_immature_cloud", "eds_map_set_immature_trace",
               "eds_map_slot_cloud")

# every symbol include/eds_hip_immdepth.h declares: immature points seeded from a depth map on the device, state beside an eds_imm (bound in immdepth.py)
IMD_EXPORTS = ("eds_imd_abi_version", "eds_imd_set_depth_map", "eds_imd_create_points_selected", "eds_imd_create_points", "eds_imd_get_nearest",
               "eds_imd_get_tree", "eds_imd_set_debug", "eds_imd_get_info")

# every symbol include/eds_hip_device.h declares: inputs that already live in device memory (its own header and ABI version)
DEV_EXPORTS = (
    "eds_dev_abi_version", "eds_dev_check_range", "eds_dev_malloc", "eds_dev_free", "eds_dev_upload", "eds_dev_download",
    "eds_dev_wait_stream", "eds_dev_signal_stream", "eds_dev_set_event_frames", "eds_dev_build_event_frames", "eds_dev_set_keyframes",
    "eds_dev_set_idepths",
)


class Header(NamedTuple):
    """one public header of include/: the names it declares, its ABI macro and the version this binding is written against"""
    file: str
    exports: tuple
    abi_macro: str
    abi_version: int


# the public headers of libeds_hip.so (eds_hip_rccl.h belongs to libeds_hip_rccl.so): a new module adds its line here
HEADERS = (
    Header("eds_hip.h", EXPORTS, "EDS_HIP_ABI_VERSION", 6),
    Header("eds_hip_depth.h", DEPTH_EXPORTS, "EDS_HIP_DEPTH_ABI_VERSION", 2),
    Header("eds_hip_klt.h", KLT_EXPORTS, "EDS_HIP_KLT_ABI_VERSION", 1),
    Header("eds_hip_epiline.h", EPI_EXPORTS, "EDS_HIP_EPILINE_ABI_VERSION", 1),
    Header("eds_hip_device.h", DEV_EXPORTS, "EDS_HIP_DEVICE_ABI_VERSION", 1),
    Header("eds_hip_kfpoints.h", KFP_EXPORTS, "EDS_HIP_KFPOINTS_ABI_VERSION", 1),
    Header("eds_hip_kfswitch.h", KFS_EXPORTS, "EDS_HIP_KFSWITCH_ABI_VERSION", 1),
    Header("eds_hip_immature.h", IMM_EXPORTS, "EDS_HIP_IMMATURE_ABI_VERSION", 1),
    Header("eds_hip_coarse.h", CT_EXPORTS, "EDS_HIP_COARSE_ABI_VERSION", 1),
    Header("eds_hip_window.h", WIN_EXPORTS, "EDS_HIP_WINDOW_ABI_VERSION", 1),
    Header("eds_hip_winsolve.h", WSV_EXPORTS, "EDS_HIP_WINSOLVE_ABI_VERSION", 1),
    Header("eds_hip_winedit.h", WED_EXPORTS, "EDS_HIP_WINEDIT_ABI_VERSION", 1),
    Header("eds_hip_winflag.h", WFL_EXPORTS, "EDS_HIP_WINFLAG_ABI_VERSION", 1),
    Header("eds_hip_activate.h", ACT_EXPORTS, "EDS_HIP_ACTIVATE_ABI_VERSION", 1),
    Header("eds_hip_select.h", SEL_EXPORTS, "EDS_HIP_SELECT_ABI_VERSION", 1),
    Header("eds_hip_init.h", INI_EXPORTS, "EDS_HIP_INIT_ABI_VERSION", 1),
    Header("eds_hip_inisetup.h", INISETUP_EXPORTS, "EDS_HIP_INISETUP_ABI_VERSION", 1),
    Header("eds_hip_undistort.h", UND_EXPORTS, "EDS_HIP_UNDISTORT_ABI_VERSION", 1),
    Header("eds_hip_map.h", MAP_EXPORTS, "EDS_HIP_MAP_ABI_VERSION", 1),
    Header("eds_hip_immdepth.h", IMD_EXPORTS, "EDS_HIP_IMMDEPTH_ABI_VERSION", 1),
)

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


class KfSelect(C.Structure):
    """``eds_kf_select`` — the arguments of KeyFrame::create that steer the point set-up (KeyFrame.cpp:333-341)."""
    _fields_ = [("method", C.c_int32), ("cell", C.c_int32), ("num_points", C.c_int32), ("sobel_ksize", C.c_int32),
                ("min_depth", C.c_double), ("max_depth", C.c_double), ("weight_threshold", C.c_double)]


class KfsDepth(C.Structure):
    """``eds_kfs_depth`` — where the depth maps of eds_kfs_build_keyframes come from (include/eds_hip_kfswitch.h)."""
    _fields_ = [("source", C.c_int32), ("src_first", C.c_int32), ("n", C.c_void_p), ("depth_xy", C.c_void_p), ("depth_idp", C.c_void_p),
                ("stride", C.c_int64), ("T7", C.c_void_p), ("K_dst", C.c_void_p)]


class KfsOut(C.Structure):
    """``eds_kfs_out`` — the optional host outputs of eds_kfs_build_keyframes."""
    _fields_ = [("n_points", C.c_void_p), ("status", C.c_void_p), ("tree_on_host", C.c_void_p), ("stride", C.c_int64),
                ("coord_xy", C.c_void_p), ("norm_xy", C.c_void_p), ("grad_xy", C.c_void_p), ("idp", C.c_void_p), ("weights", C.c_void_p)]


class DepthParams(C.Structure):
    """``eds_depth_params`` — DepthPoints::init's scalars (DepthPoints.hpp:60-75)."""
    _fields_ = [("min_depth", C.c_double), ("max_depth", C.c_double), ("threshold", C.c_double), ("init_a", C.c_double),
                ("init_b", C.c_double)]


class DepthSummary(C.Structure):
    """``eds_depth_summary`` — what one eds_depth_update did to one alignment."""
    _fields_ = [("updated", C.c_int32), ("skipped_nan", C.c_int32), ("sigma2_restored", C.c_int32), ("mu_reset", C.c_int32),
                ("converged", C.c_int32), ("pad_", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class Cfg(C.Structure):
    """``eds_trk_cfg`` — mirrors eds::tracking::Config (reference tracking/Config.hpp:40-58)."""
    _fields_ = [("device", C.c_int32), ("sampling", C.c_int32), ("solver", C.c_int32), ("exec", C.c_int32),
                ("num_blocks", C.c_int32), ("loss_type", C.c_int32), ("loss_param", C.c_double),
                ("huber_tau", C.c_double), ("lambda0", C.c_double), ("num_levels", C.c_int32),
                ("max_num_iterations", C.c_int32 * MAX_LEVELS), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double), ("nc", C.c_int32),
                ("reserved", C.c_int32 * 7)]


class Info(C.Structure):
    """``eds_trk_info`` — mirrors eds::tracking::TrackerInfo (reference tracking/Config.hpp:60-68)."""
    _fields_ = [("meas_time_us", C.c_double), ("num_points", C.c_uint32), ("num_iterations", C.c_int32),
                ("time_seconds", C.c_double), ("success", C.c_uint8), ("flags", C.c_uint8), ("pad_", C.c_uint8 * 2),
                ("termination", C.c_int32), ("num_successful_steps", C.c_int32),
                ("num_unsuccessful_steps", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("device_time_us", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class EventTimes(C.Structure):
    """``eds_event_times`` — EventFrame::create's time bookkeeping (EventFrame.cpp:313-335)."""
    _fields_ = [("first_time", C.c_int64), ("last_time", C.c_int64), ("time", C.c_int64), ("delta_time", C.c_int64),
                ("last_valid", C.c_int32), ("reserved", C.c_int32)]


def event_times(events, prev_last_time: int = 0) -> dict:
    """first / last / middle-element time stamp and their difference of a structured event array with an int64 field `ts`;
    raises EdsError(ERR_INVALID) when events[0].ts > the last time stamp, like the reference's throw.  `prev_last_time`: the previous
    slice's last_time (the reference object keeps it: a one-event slice carries it over — include/eds_hip.h)."""
    ev = np.ascontiguousarray(events)
    t = EventTimes()
    t.last_time = int(prev_last_time)
    _check(lib().eds_event_times_aos(int(ev.shape[0]), ev.ctypes.data_as(C.c_void_p), int(ev.dtype.itemsize), int(ev.dtype.fields["ts"][1]), C.byref(t)))
    return {k: getattr(t, k) for k, _ in t._fields_ if k != "reserved"}


class LaunchInfo(C.Structure):
    """``eds_trk_launch_info`` — what the last on-device solve launched (include/eds_hip.h)."""
    _fields_ = [("kernel", C.c_char * 96), ("workgroups", C.c_int32), ("cus_per_alignment", C.c_int32), ("first", C.c_int32),
                ("count", C.c_int32), ("layout", C.c_int32), ("timing_source", C.c_int32), ("span_us", C.c_double),
                ("mean_workgroup_us", C.c_double), ("covered", C.c_double), ("tail_idle_us", C.c_double)]


INFO_TEAM_TIMEOUT, INFO_TEAMS_PAUSED = 1, 2       # eds_trk_info.flags (include/eds_hip.h)
TEAM_COOLDOWN = 16                                # EDS_TEAM_COOLDOWN (csrc/eds_fused.hpp): solves without teams after a time-out


class EdsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libeds_hip error {code}: {msg}")
        self.code = code


def build_inputs() -> list:
    """The files whose age decides whether libeds_hip.so is stale: every .hip and .hpp of csrc, every header of HEADERS."""
    return ([os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp"))] +
            [os.path.join(INCLUDE, h.file) for h in HEADERS])


def build(force: bool = False) -> str:
    """Compile libeds_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = build_inputs()
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    rccl_lib = os.path.join(CSRC, "libeds_hip_rccl.so")       # include/eds_hip_rccl.h: the RCCL gather for a C / C++ caller (its own library)
    rccl_src = [os.path.join(CSRC, "eds_gather.hip"), os.path.join(INCLUDE, "eds_hip_rccl.h")]
    stale_rccl = (not os.path.exists(rccl_lib)) or any(os.path.getmtime(s) > os.path.getmtime(rccl_lib) for s in rccl_src)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-j4", "-s", "libeds_hip.so"])
    if force or stale_rccl:
        subprocess.check_call(["make", "-C", CSRC, "-s", "libeds_hip_rccl.so"])
    return LIB_PATH


_lib = None
# PyTorch-ROCm ships its own libamdhip64.so.7 and libeds_hip.so is linked against /opt/rocm's: one process holds ONE copy of a SONAME,
# whichever is loaded first.  torch works only on its own, libeds_hip on either — so a process that uses torch.cuda as well must
# import torch before the first call into this module (bench.py and BatchTracker do; batch.gather_results checks).
torch_loaded_first = None


def lib():
    """Loads the library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EdsError(ERR_NO_DEVICE, f"{LIB_PATH} is missing — run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        global torch_loaded_first
        import sys
        torch_loaded_first = "torch" in sys.modules
        L = C.CDLL(LIB_PATH)
        L.eds_last_error.restype = C.c_char_p
        L.eds_trk_create.argtypes = [C.POINTER(Cfg), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.eds_trk_destroy.argtypes = [C.c_void_p]
        L.eds_trk_destroy.restype = None
        L.eds_trk_cfg_default.argtypes = [C.POINTER(Cfg)]
        L.eds_trk_cfg_default.restype = None
        L.eds_trk_set_config.argtypes = [C.c_void_p, C.POINTER(Cfg)]
        L.eds_trk_get_config.argtypes = [C.c_void_p, C.POINTER(Cfg)]
        L.eds_trk_set_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_double,
                                           C.c_double, C.c_double]
        L.eds_trk_set_idepth.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.eds_trk_set_idepth_strided.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int]
        L.eds_trk_set_event_frame.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_trk_set_event_frame_f32.argtypes = [C.c_void_p, C.c_int, _fp]
        L.eds_trk_set_event_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.eds_trk_set_event_frames_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.eds_trk_set_state.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
        L.eds_trk_get_state.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
        L.eds_trk_set_undistort_map.argtypes = [C.c_void_p, _fp, _fp]
        L.eds_trk_build_event_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16),
                                                C.POINTER(C.c_uint8), C.c_int, C.c_double, C.c_int, _dp]
        L.eds_trk_get_event_frame.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_trk_set_undistort_map_sized.argtypes = [C.c_void_p, _fp, _fp, C.c_int, C.c_int]
        L.eds_trk_build_event_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16),
                                                 C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_double, C.c_int, _dp]
        L.eds_trk_build_event_frames_aos.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, C.c_int, C.c_double, C.c_int, _dp]
        L.eds_trk_build_event_frames_aos_timed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                           C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _dp, C.POINTER(EventTimes)]
        L.eds_event_times_aos.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(EventTimes)]
        L.eds_trk_build_event_frame_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16),
                                                      C.POINTER(C.c_uint8), C.c_int, C.c_double, C.c_int, _dp]
        L.eds_trk_share_event_frame.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.eds_trk_set_states.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
        L.eds_trk_get_states.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
        L.eds_trk_get_results.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.eds_trk_eval.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp]
        L.eds_trk_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(Info)]
        L.eds_trk_optimize_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.eds_trk_optimize_batch_wait.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.eds_trk_sync.argtypes = [C.c_void_p]
        L.eds_trk_get_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(Info)]
        L.eds_trk_get_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _ip]
        L.eds_trk_get_residuals.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_trk_loss_param.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.eds_trk_loss_param_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp]
        L.eds_trk_update_points.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp]
        L.eds_trk_update_points_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp]
        L.eds_kf_select_default.argtypes = [C.POINTER(KfSelect)]
        L.eds_kf_select_default.restype = None
        L.eds_trk_build_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(KfSelect), C.c_int, _dp, _dp,
                                             C.c_double, C.c_double, C.c_double, C.c_double, _ip]
        L.eds_trk_get_keyframe_points.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp]
        L.eds_trk_build_keyframe_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(KfSelect),
                                                   C.c_int, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double, _ip]
        L.eds_trk_timer_start.argtypes = [C.c_void_p]
        L.eds_trk_timer_stop.argtypes = [C.c_void_p, _fp]
        L.eds_trk_bench_eval.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp]
        L.eds_trk_bench_live.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _dp]
        L.eds_trk_bench_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _dp]
        L.eds_trk_bench_kernel_cold.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp]
        L.eds_trk_hbm_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int, _fp, _fp]
        L.eds_pyr_create.argtypes = [C.POINTER(Cfg), C.c_int, _ip, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.eds_pyr_destroy.argtypes = [C.c_void_p]
        L.eds_pyr_destroy.restype = None
        L.eds_pyr_set_config.argtypes = [C.c_void_p, C.POINTER(Cfg)]
        L.eds_pyr_level_intrinsics.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, _dp]
        L.eds_pyr_set_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double]
        L.eds_pyr_set_event_frame.argtypes = [C.c_void_p, _dp]
        L.eds_pyr_build_event_frame.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8),
                                                C.c_double, C.c_int, _dp]
        L.eds_pyr_level_size.argtypes = [C.c_void_p, C.c_int, _ip, _ip]
        L.eds_pyr_get_level_frame.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_pyr_optimize.argtypes = [C.c_void_p, _dp, _dp, _dp, C.POINTER(Info)]
        L.eds_pyr_create_batch.argtypes = [C.POINTER(Cfg), C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.eds_pyr_set_keyframe_slot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double]
        L.eds_pyr_set_event_frame_slot.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_pyr_optimize_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(Info)]
        L.eds_trk_last_launch.argtypes = [C.c_void_p, C.POINTER(LaunchInfo)]
        L.eds_trk_set_knob.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.eds_trk_get_strips_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), _ip, _ip]
        L.eds_pyr_get_residuals.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_depth_params_default.argtypes = [C.POINTER(DepthParams)]
        L.eds_depth_params_default.restype = None
        L.eds_depth_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(DepthParams), C.c_int, _dp, C.c_int]
        L.eds_depth_update.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, C.POINTER(DepthSummary)]
        L.eds_depth_get.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_uint8)]
        L.eds_depth_set.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_depth_get_idepth.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_depth_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        for fn in (L.eds_klt_track_points, L.eds_klt_track_points_pyr):
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip]
        L.eds_klt_get.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.eds_epi_track_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp,
                                           _ip, _ip]
        L.eds_epi_get.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_epi_get_model.argtypes = [C.c_void_p, C.c_int, _dp]
        L.eds_epi_depth_update.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int, C.POINTER(DepthSummary)]
        L.eds_kfp_refine_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _ip, _ip]
        L.eds_kfp_clean_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, _ip, _ip]
        L.eds_kfp_erase_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), _ip, _ip]
        L.eds_kfp_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _ip]
        L.eds_kfp_project_depth_map.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _ip]
        L.eds_kfs_build_tree.argtypes = [C.c_void_p, C.c_int, _ip, C.c_void_p, C.c_int64, _ip, C.POINTER(C.c_uint8)]
        L.eds_kfs_build_keyframes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(KfSelect), _dp,
                                              C.POINTER(KfsDepth), C.POINTER(KfsOut)]
        L.eds_kfs_build_keyframes_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(KfSelect), _dp,
                                                  C.POINTER(KfsDepth), C.POINTER(KfsOut)]
        L.eds_dev_check_range.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
        L.eds_dev_malloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.eds_dev_free.argtypes = [C.c_void_p]
        L.eds_dev_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.eds_dev_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.eds_dev_wait_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.eds_dev_signal_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.eds_dev_set_event_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64]
        L.eds_dev_build_event_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                                 C.c_int, _dp]
        L.eds_dev_set_keyframes.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _dp]
        L.eds_dev_set_idepths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int]
        if L.eds_trk_cfg_size() != C.sizeof(Cfg) or L.eds_trk_info_size() != C.sizeof(Info):
            raise EdsError(ERR_INVALID, "ctypes struct layout disagrees with include/eds_hip.h")
        _lib = L
    return _lib


def last_error() -> str:
    return (lib().eds_last_error() or b"").decode()


def _check(rc):
    if rc != EDS_OK:
        raise EdsError(rc, last_error())


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def vp(a):
    """a numpy array's memory as a ``void*``; None stays None"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bind(exports, signatures):
    """The loaded library, after one check that it exports every name of `exports`, with the prototypes of `signatures` set:
    ``name -> argtypes``, or ``name -> (argtypes, restype)`` where the function does not return an int."""
    L = lib()
    missing = [s for s in exports if not hasattr(L, s)]
    if missing:
        raise EdsError(ERR_INVALID, f"{LIB_PATH} does not export {missing}")
    for name, sig in signatures.items():
        if isinstance(sig, tuple):
            getattr(L, name).argtypes, getattr(L, name).restype = sig
        else:
            getattr(L, name).argtypes = sig
    return L


class ParamStruct(C.Structure):
    """A ``*_params`` record of the C ABI."""

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}

    def update(self, **over):
        """sets the named members (KeyError for a name the record does not have); returns the record"""
        for k, v in over.items():
            if not hasattr(self, k):
                raise KeyError(k)
            setattr(self, k, v)
        return self


class OwnedHandle:
    """An object that owns one handle of the C ABI in ``_h``: ``close`` destroys it once, so do garbage collection and the end of a
    ``with`` block.  ``_destroy`` names the C function (its prototype is set by the module's ``bind``)."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def is_device_source(obj) -> bool:
    """device memory as the bindings take it: ``__cuda_array_interface__``, or a raw ``(ptr, shape, strides, dtype)`` tuple"""
    return hasattr(obj, "__cuda_array_interface__") or (isinstance(obj, tuple) and len(obj) == 4 and isinstance(obj[0], int))


def _rows(a, count, width):
    """per-slot rows -> (contiguous count x stride [x width] float64 array, stride): an array is taken as it is, a list of
    per-slot arrays of different lengths is padded to the longest"""
    if isinstance(a, (list, tuple)):
        stride = max(1, max(len(r) for r in a))
        t = np.zeros((count, stride) + ((width,) if width > 1 else ()))
        for b, r in enumerate(a):
            t[b, :len(r)] = r
        return t, stride
    t = _f64(a)
    if t.ndim == (1 if width == 1 else 2):
        t = t[None]
    return np.ascontiguousarray(t), int(t.shape[1])


# -- arrays in device memory (include/eds_hip_device.h) --------------------------------------------------------------------------
# Everything below up to DeviceArray is pure Python: it reads ``__cuda_array_interface__`` (torch device tensors on ROCm have it,
# DeviceArray has it) or a raw ``(ptr, shape, strides, dtype)`` tuple and raises ValueError before the library is called.
def is_device_array(obj) -> bool:
    return hasattr(obj, "__cuda_array_interface__")


def device_array_info(obj):
    """``(ptr, shape, strides in ELEMENTS, numpy dtype)`` of an object with ``__cuda_array_interface__`` or of a raw
    ``(ptr, shape, strides in bytes or None, dtype)`` tuple.  ValueError: no pointer, or a byte stride that is no whole number of
    elements."""
    if isinstance(obj, tuple) and len(obj) == 4 and not hasattr(obj, "__cuda_array_interface__"):
        ptr, shape, strides, dtype = obj
        dt = np.dtype(dtype)
    else:
        try:
            cai = obj.__cuda_array_interface__
        except AttributeError:
            raise ValueError("not a device array: no __cuda_array_interface__ (and not a (ptr, shape, strides, dtype) tuple)") from None
        ptr, shape, strides = cai["data"][0], cai["shape"], cai.get("strides")
        dt = np.dtype(cai["typestr"])
    shape = tuple(int(n) for n in shape)
    if dt.byteorder == ">":
        raise ValueError("big-endian device array")
    if not ptr and int(np.prod(shape, dtype=np.int64)) > 0:
        raise ValueError("device array without a pointer")
    if strides is None:                     # C-contiguous
        st, acc = [], 1
        for n in reversed(shape):
            st.append(acc)
            acc *= max(n, 1)
        est = tuple(reversed(st))
    else:
        if len(strides) != len(shape):
            raise ValueError("strides and shape have different lengths")
        for b in strides:
            if int(b) % dt.itemsize:
                raise ValueError(f"a stride of {int(b)} bytes is no whole number of {dt.name} elements")
        est = tuple(int(b) // dt.itemsize for b in strides)
    return int(ptr or 0), shape, est, dt


def device_frames_args(obj, H, W):
    """Arguments of eds_dev_set_event_frames for `obj`: ``(ptr, count, dtype code, frame_stride, row_stride)``, strides in elements.
    `obj`: count x H x W (or H x W: one frame), float32 or float64, last dimension contiguous, rows and frames not overlapping."""
    ptr, shape, est, dt = device_array_info(obj)
    if len(shape) == 2:
        shape, est = (1,) + shape, (0,) + est
    if len(shape) != 3:
        raise ValueError(f"event frames must be count x H x W (or H x W), not {len(shape)}-dimensional")
    if dt == np.float32:
        code = IMG_F32
    elif dt == np.float64:
        code = IMG_F64
    else:
        raise ValueError(f"event frames must be float32 or float64, not {dt.name}")
    count = shape[0]
    if shape[1:] != (int(H), int(W)):
        raise ValueError(f"frames of {shape[1]} x {shape[2]} do not fit a handle of {H} x {W}")
    if count < 1:
        raise ValueError("no frame")
    if est[2] != 1:
        raise ValueError("the last dimension must be contiguous (a stride of one element)")
    row = est[1]
    if row < W:
        raise ValueError("rows overlap or run backwards (row stride < W)")
    need = (H - 1) * row + W
    frame = est[0] if count > 1 else need
    if frame < need:
        raise ValueError("frames overlap or run backwards (frame stride < (H - 1) * row stride + W)")
    return ptr, count, code, frame, row


def _device_rows(obj, count, width, name):
    """(ptr, points per row, point stride between rows) of a float64 device array count x S [x width] whose rows are dense"""
    ptr, shape, est, dt = device_array_info(obj)
    if dt != np.float64:
        raise ValueError(f"{name} must be float64, not {dt.name}")
    want = 2 if width == 1 else 3
    if len(shape) == want - 1:
        shape, est = (1,) + shape, (0,) + est
    if len(shape) != want or shape[0] != count or (width > 1 and shape[2] != width):
        raise ValueError(f"{name} must be count x S" + (f" x {width}" if width > 1 else "") + f" with count = {count}, not {shape}")
    if est[-1] != 1 or (width > 1 and est[1] != width):
        raise ValueError(f"the rows of {name} must be contiguous")
    S = shape[1]
    if count > 1 and (est[0] % width or est[0] // width < S):
        raise ValueError(f"the rows of {name} overlap or are not a whole number of points apart")
    return ptr, S, (est[0] // width if count > 1 else S)


def _kfs_device_images(obj, H, W):
    """Arguments of eds_kfs_build_keyframes_dev for `obj`: ``(ptr, count, dtype code, frame_stride, row_stride)``, strides in elements.
    `obj`: count x H x W (or H x W), uint8 / float32 / float64, last dimension contiguous, rows and frames not overlapping."""
    ptr, shape, est, dt = device_array_info(obj)
    if len(shape) == 2:
        shape, est = (1,) + shape, (0,) + est
    codes = {np.dtype(np.uint8): IMG_U8, np.dtype(np.float32): IMG_F32, np.dtype(np.float64): IMG_F64}
    if dt not in codes:
        raise ValueError(f"keyframe images must be uint8, float32 or float64, not {dt.name}")
    if len(shape) != 3 or shape[0] < 1 or shape[1:] != (int(H), int(W)):
        raise ValueError(f"keyframe images must be count x {H} x {W}, not {shape}")
    if est[2] != 1 or est[1] < W:
        raise ValueError("the last dimension must be contiguous and rows must not overlap")
    need = (H - 1) * est[1] + W
    frame = est[0] if shape[0] > 1 else need
    if frame < need:
        raise ValueError("frames overlap or run backwards")
    return ptr, shape[0], codes[dt], frame, est[1]


def _stream_ptr(stream):
    """a hipStream_t as an integer: None / 0 is the null stream; an int, or an object with ``.cuda_stream`` (torch.cuda.Stream)"""
    if stream is None:
        return None
    v = int(getattr(stream, "cuda_stream", stream))
    return v or None


class DeviceArray:
    """A dense array in device memory, owned through ``eds_dev_malloc`` (the HIP runtime libeds_hip.so itself is bound to), for
    callers without a HIP binding and for the tests.  Has ``__cuda_array_interface__``; ``view`` describes a strided window of it."""

    def __init__(self, shape, dtype, device=0):
        self.shape = tuple(int(n) for n in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.device = int(device)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(lib().eds_dev_malloc(self.device, max(self.nbytes, 1), C.byref(p)))
        self.ptr = int(p.value)

    @classmethod
    def from_numpy(cls, a, device=0):
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype, device)
        if d.nbytes:
            _check(lib().eds_dev_upload(C.c_void_p(d.ptr), a.ctypes.data_as(C.c_void_p), d.nbytes))
        return d

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            _check(lib().eds_dev_download(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), self.nbytes))
        return out

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "strides": None, "version": 3}

    def view(self, shape, strides=None, offset=0):
        """A window of this buffer: `shape`, `strides` in BYTES (None: dense), starting `offset` bytes in.  Keeps the buffer alive."""
        return DeviceView(self, tuple(int(n) for n in shape), None if strides is None else tuple(int(b) for b in strides), int(offset))

    def free(self):
        if getattr(self, "ptr", 0):
            lib().eds_dev_free(C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView:
    """What DeviceArray.view returns: ``__cuda_array_interface__`` of a strided window; owns nothing."""

    def __init__(self, base, shape, strides, offset):
        self.base, self.shape, self.strides, self.offset = base, shape, strides, offset

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.base.dtype.str, "data": (self.base.ptr + self.offset, False), "strides": self.strides,
                "version": 3}


def tree_capacity() -> int:
    """``eds_kfs_tree_capacity``: points per depth map the device builds the k-d tree of; larger maps take the host build."""
    return int(lib().eds_kfs_tree_capacity())


def kfs_chunk_size() -> int:
    """``eds_kfs_chunk_size``: slots that build_keyframes queues between two waits on the stream."""
    return int(lib().eds_kfs_chunk_size())


def check_range(ptr, nbytes, device=0) -> int:
    """``eds_dev_check_range``: EDS_OK or ERR_INVALID (the reason: last_error()).  Launches nothing."""
    return int(lib().eds_dev_check_range(int(device), C.c_void_p(int(ptr) or None), int(nbytes)))


def default_config(**kw) -> Cfg:
    cfg = Cfg()
    lib().eds_trk_cfg_default(C.byref(cfg))
    for k, v in kw.items():
        if k == "max_num_iterations":
            v = [int(v)] * MAX_LEVELS if np.isscalar(v) else list(v) + [list(v)[-1]] * (MAX_LEVELS - len(v))
            cfg.max_num_iterations = (C.c_int32 * MAX_LEVELS)(*v[:MAX_LEVELS])
        else:
            setattr(cfg, k, v)
    return cfg


class Handle:
    """RAII wrapper of ``eds_trk*``: ``batch`` alignment slots on one GPU / one HIP stream."""

    def __init__(self, cfg: Cfg, batch: int, max_points: int, H: int, W: int):
        self._h = C.c_void_p()
        self.batch, self.max_points, self.H, self.W = int(batch), int(max_points), int(H), int(W)
        _check(lib().eds_trk_create(C.byref(cfg), self.batch, self.max_points, self.H, self.W, C.byref(self._h)))
        self._N = [0] * self.batch

    def close(self):
        if self._h:
            lib().eds_trk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -------------------------------------------------------------------
    def set_config(self, cfg: Cfg):
        _check(lib().eds_trk_set_config(self._h, C.byref(cfg)))

    def get_config(self) -> Cfg:
        cfg = Cfg()
        _check(lib().eds_trk_get_config(self._h, C.byref(cfg)))
        return cfg

    # -- inputs --------------------------------------------------------------------------
    def set_keyframe(self, slot, norm_coord, grad, idp, weights, fx, fy, cx, cy):
        nc, g, d, w = _f64(norm_coord), _f64(grad), _f64(idp), _f64(weights)
        N = int(d.shape[0])
        if nc.shape != (N, 2) or g.shape != (N, 2) or w.shape != (N,):
            raise EdsError(ERR_INVALID, "keyframe arrays have inconsistent shapes")
        _check(lib().eds_trk_set_keyframe(self._h, slot, N, _p(nc), _p(g), _p(d), _p(w), fx, fy, cx, cy))
        self._N[slot] = N

    def set_alignment(self, slot, al):
        """Convenience: upload an ``Alignment`` (synth.py) and seed its start state."""
        self.set_keyframe(slot, al.norm_coord, al.grad, al.idp, al.weights, al.fx, al.fy, al.cx, al.cy)
        self.set_event_frame(slot, al.frame)
        self.set_state(slot, al.p0, al.q0, al.v0)

    def set_idepth(self, slot, idp):
        d = _f64(idp)
        _check(lib().eds_trk_set_idepth(self._h, slot, int(d.shape[0]), _p(d)))

    def set_idepth_strided(self, slot, table, column=0):
        """Inverse depths as column `column` of a row-major N x k table of doubles (DepthPoints keeps N x 4)."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        _check(lib().eds_trk_set_idepth_strided(self._h, slot, int(t.shape[0]), t[:, column:].ctypes.data_as(_dp), int(t.shape[1])))

    def set_event_frame(self, slot, frame):
        fr = np.asarray(frame)
        if fr.size != self.H * self.W:
            raise EdsError(ERR_INVALID, "event frame size != H*W")
        if fr.dtype == np.float32:
            fr = np.ascontiguousarray(fr)
            _check(lib().eds_trk_set_event_frame_f32(self._h, slot, fr.ctypes.data_as(_fp)))
        else:
            fr = _f64(fr)
            _check(lib().eds_trk_set_event_frame(self._h, slot, _p(fr)))

    def set_event_frames(self, first, frames):
        """Many host frames in ONE call (eds_trk_set_event_frames / _f32): frames[i] -> slot first + i; all fp64 or all fp32, each H x W."""
        arrs = [np.ascontiguousarray(f) for f in frames]
        f32 = all(a.dtype == np.float32 for a in arrs)
        if not f32:
            arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in arrs]
        for a in arrs:
            if a.size != self.H * self.W:
                raise ValueError("frame size does not match the handle")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        fn = lib().eds_trk_set_event_frames_f32 if f32 else lib().eds_trk_set_event_frames
        _check(fn(self._h, int(first), len(arrs), ptrs))

    # -- inputs that already live in device memory (include/eds_hip_device.h) -----------------------------------------------
    def wait_stream(self, stream=None):
        """The handle's stream waits for everything queued on `stream` so far (an int, an object with ``.cuda_stream``, None: the null stream)."""
        _check(lib().eds_dev_wait_stream(self._h, _stream_ptr(stream)))

    def signal_stream(self, stream=None):
        """`stream` waits for everything queued on the handle's stream so far: a source buffer may be reused behind this."""
        _check(lib().eds_dev_signal_stream(self._h, _stream_ptr(stream)))

    def set_event_frames_device(self, first, frames):
        """count x H x W (or H x W) float32 / float64 frames in device memory -> slots first .. first + count - 1, one launch on the
        handle's stream (eds_dev_set_event_frames).  `frames`: anything with ``__cuda_array_interface__``, or (ptr, shape, strides, dtype)."""
        ptr, count, code, fs, rs = device_frames_args(frames, self.H, self.W)
        _check(lib().eds_dev_set_event_frames(self._h, int(first), count, code, C.c_void_p(ptr), fs, rs))

    def build_event_frames_device(self, first_slot, offsets, x, y, polarity, level=0, blur_sigma=0.5, use_exp_weights=True):
        """build_event_frame_batch with the concatenated event arrays (uint16 x, y, uint8 polarity) in device memory; slice b is
        events offsets[b] .. offsets[b + 1] - 1.  Returns the norms."""
        offs = np.ascontiguousarray(offsets, dtype=np.int32)
        if offs.ndim != 1 or offs.shape[0] < 2:
            raise ValueError("offsets: count + 1 integers")
        ptrs = []
        for a, dt, name in ((x, np.uint16, "x"), (y, np.uint16, "y"), (polarity, np.uint8, "polarity")):
            ptr, shape, est, d = device_array_info(a)
            if d != dt or len(shape) != 1 or est[0] != 1:
                raise ValueError(f"{name} must be a contiguous 1-D {np.dtype(dt).name} device array")
            if shape[0] < int(offs[-1]):
                raise ValueError(f"{name} holds {shape[0]} events, the offsets ask for {int(offs[-1])}")
            ptrs.append(C.c_void_p(ptr or None))
        norms = np.zeros(offs.shape[0] - 1)
        _check(lib().eds_dev_build_event_frames(self._h, int(first_slot), offs.shape[0] - 1, offs.ctypes.data_as(_ip), *ptrs, int(level),
                                                float(blur_sigma), int(bool(use_exp_weights)), _p(norms)))
        return norms

    def set_keyframes_device(self, first, N, norm_coord, grad, idp, weights, K):
        """set_keyframe for slots first .. first + len(N) - 1 from float64 device arrays: norm_coord, grad count x S x 2, idp, weights
        count x S (rows the same number of points apart in all four), N[b] points used of row b, K count x (fx, fy, cx, cy)."""
        n = np.ascontiguousarray(N, dtype=np.int32).reshape(-1)
        count = int(n.shape[0])
        k = _f64(K).reshape(-1)
        if k.shape[0] != 4 * count:
            raise ValueError("K must be count x 4 (fx, fy, cx, cy)")
        rows = [_device_rows(a, count, w, name) for a, w, name in ((norm_coord, 2, "norm_coord"), (grad, 2, "grad"), (idp, 1, "idp"),
                                                                   (weights, 1, "weights"))]
        if len({r[2] for r in rows}) != 1:
            raise ValueError("the four keyframe arrays must have the same point stride between alignments")
        if count and int(n.max()) > min(r[1] for r in rows):
            raise ValueError("N exceeds the points per row of the arrays")
        if count and (int(n.min()) < 1 or int(n.max()) > self.max_points):
            raise ValueError("N out of range for this handle")
        _check(lib().eds_dev_set_keyframes(self._h, int(first), count, n.ctypes.data_as(_ip), *[C.c_void_p(r[0] or None) for r in rows],
                                           rows[0][2], _p(k)))
        for b in range(count):
            self._N[int(first) + b] = int(n[b])

    def set_idepths_device(self, first, idp):
        """set_idepth for slots first .. first + count - 1 from a float64 device array count x S (or count x S x k: column 0 of an
        S x k table per slot, as set_idepth_strided)."""
        ptr, shape, est, dt = device_array_info(idp)
        if dt != np.float64:
            raise ValueError(f"idp must be float64, not {dt.name}")
        if len(shape) == 3:
            shape, est = shape[:2], est[:2]
        if len(shape) != 2:
            raise ValueError("idp must be count x S (or count x S x k)")
        count, S = shape
        es = est[1]
        if count < 1 or es < 1 or (count > 1 and (est[0] % es or est[0] // es < S)):
            raise ValueError("idp: rows must be a whole, non-overlapping number of points apart")
        if max(self._N[int(first):int(first) + count] + [0]) > S:
            raise ValueError("idp holds fewer points per row than the slots do")
        _check(lib().eds_dev_set_idepths(self._h, int(first), count, C.c_void_p(ptr or None), est[0] // es if count > 1 else S, es))

    def set_undistort_map(self, mapx=None, mapy=None):
        if mapx is None:
            _check(lib().eds_trk_set_undistort_map(self._h, None, None))
            return
        mx, my = np.ascontiguousarray(mapx, dtype=np.float32), np.ascontiguousarray(mapy, dtype=np.float32)
        if mx.size != self.H * self.W or my.size != self.H * self.W:
            raise EdsError(ERR_INVALID, "undistortion map size != H*W")
        _check(lib().eds_trk_set_undistort_map(self._h, mx.ctypes.data_as(_fp), my.ctypes.data_as(_fp)))

    def build_event_frame(self, slot, x, y, polarity, level=0, blur_sigma=0.5, use_exp_weights=True):
        """EventFrame::create on the device; returns the Frobenius norm the frame was divided by."""
        ex = np.ascontiguousarray(x, dtype=np.uint16)
        ey = np.ascontiguousarray(y, dtype=np.uint16)
        pol = np.ascontiguousarray(polarity, dtype=np.uint8)
        norm = C.c_double(0.0)
        _check(lib().eds_trk_build_event_frame(self._h, slot, int(ex.shape[0]), ex.ctypes.data_as(C.POINTER(C.c_uint16)),
                                               ey.ctypes.data_as(C.POINTER(C.c_uint16)), pol.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               int(level), float(blur_sigma), int(bool(use_exp_weights)),
                                               C.cast(C.byref(norm), _dp)))
        return norm.value

    def build_event_frames(self, first_slot, num_levels, x, y, polarity, sensor_size=None, blur_sigma=0.5, use_exp_weights=True):
        """All `num_levels` frames of one event slice from a single vote (EventFrame::create), level i into slot first_slot + i;
        sensor_size = (H, W) of the events / LUT when it differs from the handle's frame size (out_scale != 1).  Returns the norms."""
        x = np.ascontiguousarray(x, dtype=np.uint16); y = np.ascontiguousarray(y, dtype=np.uint16)
        pol = np.ascontiguousarray(polarity, dtype=np.uint8)
        sH, sW = (0, 0) if sensor_size is None else sensor_size
        norms = np.zeros(num_levels)
        _check(lib().eds_trk_build_event_frames(self._h, int(first_slot), int(num_levels), int(x.shape[0]),
                                                x.ctypes.data_as(C.POINTER(C.c_uint16)), y.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                pol.ctypes.data_as(C.POINTER(C.c_uint8)), int(sH), int(sW), float(blur_sigma),
                                                int(bool(use_exp_weights)), _p(norms)))
        return norms

    def build_event_frames_aos(self, first_slot, num_levels, events, sensor_size=None, blur_sigma=0.5, use_exp_weights=True):
        """`events`: a numpy structured array with fields x, y (uint16) and polarity (1 byte) — e.g. the memory of a
        std::vector<base::samples::Event>."""
        ev = np.ascontiguousarray(events)
        f = ev.dtype.fields
        sH, sW = sensor_size if sensor_size is not None else (0, 0)
        norms = np.zeros(num_levels)
        _check(lib().eds_trk_build_event_frames_aos(self._h, int(first_slot), int(num_levels), int(ev.shape[0]), ev.ctypes.data_as(C.c_void_p),
                                                    int(ev.dtype.itemsize), int(f["x"][1]), int(f["y"][1]), int(f["polarity"][1]), int(sH), int(sW),
                                                    float(blur_sigma), int(bool(use_exp_weights)), _p(norms)))
        return norms

    def build_event_frames_aos_timed(self, first_slot, num_levels, events, sensor_size=None, blur_sigma=0.5, use_exp_weights=True):
        """As build_event_frames_aos on records that also carry `ts` (int64): returns (norms, times dict); the time check comes first."""
        ev = np.ascontiguousarray(events)
        f = ev.dtype.fields
        sH, sW = sensor_size if sensor_size is not None else (0, 0)
        norms = np.zeros(num_levels)
        t = EventTimes()
        _check(lib().eds_trk_build_event_frames_aos_timed(self._h, int(first_slot), int(num_levels), int(ev.shape[0]), ev.ctypes.data_as(C.c_void_p),
                                                          int(ev.dtype.itemsize), int(f["x"][1]), int(f["y"][1]), int(f["polarity"][1]), int(f["ts"][1]),
                                                          int(sH), int(sW), float(blur_sigma), int(bool(use_exp_weights)), _p(norms), C.byref(t)))
        return norms, {k: getattr(t, k) for k, _ in t._fields_ if k != "reserved"}

    def build_event_frame_batch(self, first_slot, slices, level=0, blur_sigma=0.5, use_exp_weights=True):
        """`slices`: one (x, y, polarity) triple per slot, first_slot onwards; returns the norms."""
        offs = np.zeros(len(slices) + 1, dtype=np.int32)
        for b, (x, _, _) in enumerate(slices):
            offs[b + 1] = offs[b] + len(x)
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(sl[k], dtype=dt) for sl in slices]) if len(slices) else np.zeros(0, dt), dtype=dt)
        x, y, pol = cat(0, np.uint16), cat(1, np.uint16), cat(2, np.uint8)
        norms = np.zeros(len(slices))
        _check(lib().eds_trk_build_event_frame_batch(self._h, int(first_slot), len(slices), offs.ctypes.data_as(_ip),
                                                     x.ctypes.data_as(C.POINTER(C.c_uint16)), y.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                     pol.ctypes.data_as(C.POINTER(C.c_uint8)), int(level), float(blur_sigma),
                                                     int(bool(use_exp_weights)), _p(norms)))
        return norms

    def set_undistort_map_sized(self, mapx, mapy, sensor_size):
        mx = np.ascontiguousarray(mapx, dtype=np.float32); my = np.ascontiguousarray(mapy, dtype=np.float32)
        assert mx.shape == tuple(sensor_size) and my.shape == tuple(sensor_size)
        _check(lib().eds_trk_set_undistort_map_sized(self._h, mx.ctypes.data_as(_fp), my.ctypes.data_as(_fp), int(sensor_size[0]), int(sensor_size[1])))

    def share_event_frame(self, slot, src_slot):
        _check(lib().eds_trk_share_event_frame(self._h, int(slot), int(src_slot)))

    def get_event_frame(self, slot):
        fr = np.zeros((self.H, self.W))
        _check(lib().eds_trk_get_event_frame(self._h, slot, _p(fr)))
        return fr

    def set_state(self, slot, p=None, q=None, v=None):
        p = None if p is None else _f64(p)
        q = None if q is None else _f64(q)
        v = None if v is None else _f64(v)
        _check(lib().eds_trk_set_state(self._h, slot, _p(p), _p(q), _p(v)))

    def get_state(self, slot):
        p, q, v = np.zeros(3), np.zeros(4), np.zeros(6)
        _check(lib().eds_trk_get_state(self._h, slot, _p(p), _p(q), _p(v)))
        return p, q, v

    def set_states(self, first, p=None, q=None, v=None):
        """Bulk seed of slots [first, first+count): p count x 3, q count x 4, v count x 6."""
        arrs = [None if a is None else _f64(a) for a in (p, q, v)]
        count = next(a.shape[0] for a in arrs if a is not None)
        _check(lib().eds_trk_set_states(self._h, first, count, *[_p(a) for a in arrs]))

    def get_states(self, first=0, count=None):
        count = self.batch - first if count is None else count
        p, q, v = np.zeros((count, 3)), np.zeros((count, 4)), np.zeros((count, 6))
        _check(lib().eds_trk_get_states(self._h, first, count, _p(p), _p(q), _p(v)))
        return p, q, v

    def results(self, first=0, count=None, out=None):
        """count x 16 table: p[3] q[4] v[6] final_cost iterations success.  `out`: a C-contiguous float64 array of that shape to fill
        (a caller that steps in a loop keeps one: a fresh half-megabyte array per call is an mmap and its page faults)."""
        count = self.batch - first if count is None else count
        if out is None:
            out = np.empty((count, 16))         # (the call fills every column)
        elif out.shape != (count, 16) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise EdsError(ERR_INVALID, "results(out=...): a C-contiguous float64 array of shape (count, 16)")
        _check(lib().eds_trk_get_results(self._h, first, count, _p(out)))
        return out

    # -- evaluation / solve --------------------------------------------------------------
    def eval(self, slot, p, q, v, ncols=6, want_jacobian=True):
        N = self._N[slot]
        p, q, v = _f64(p), _f64(q), _f64(v)
        r = np.zeros(N)
        J = np.zeros((N, ncols)) if want_jacobian else None
        JtJ, Jtr, cost = np.zeros((ncols, ncols)), np.zeros(ncols), C.c_double(0.0)
        _check(lib().eds_trk_eval(self._h, slot, _p(p), _p(q), _p(v), ncols, _p(r), _p(J), _p(JtJ), _p(Jtr),
                                  C.cast(C.byref(cost), _dp)))
        return dict(r=r, J=J, JtJ=JtJ, Jtr=Jtr, cost=cost.value)

    def optimize(self, slot, level=0, p=None, q=None, v=None):
        """Tracker::optimize for one slot.  Returns (p, q, v, info dict); raises EdsError(ERR_NOT_USABLE)."""
        if p is None or q is None or v is None:         # (the stored state only where the caller leaves one out: a call less on the live path)
            sp, sq, sv = self.get_state(slot)
        p = sp if p is None else _f64(p).copy()
        q = sq if q is None else _f64(q).copy()
        v = sv if v is None else _f64(v).copy()
        info = Info()
        _check(lib().eds_trk_optimize(self._h, slot, level, _p(p), _p(q), _p(v), C.byref(info)))
        return p, q, v, info.as_dict()

    def optimize_batch(self, level=0, first=0, count=None, sync=True):
        count = self.batch - first if count is None else count
        if sync:            # ABI 6: launch + wait + collect in one call (no interpreter between them)
            _check(lib().eds_trk_optimize_batch_wait(self._h, level, first, count))
        else:
            _check(lib().eds_trk_optimize_batch(self._h, level, first, count))

    def sync(self):
        _check(lib().eds_trk_sync(self._h))

    def info(self, slot):
        info = Info()
        _check(lib().eds_trk_get_info(self._h, slot, C.byref(info)))
        return info.as_dict()

    def trace(self, slot, max_iters=128):
        inc, cost, acc = np.zeros((max_iters, 6)), np.zeros(max_iters), np.zeros(max_iters, dtype=np.int32)
        n = lib().eds_trk_get_trace(self._h, slot, max_iters, _p(inc), _p(cost), acc.ctypes.data_as(_ip))
        if n < 0:
            _check(n)
        return dict(increments=inc[:n], costs=cost[:n], accepted=acc[:n])

    def residuals(self, slot):
        r = np.zeros(self._N[slot])
        _check(lib().eds_trk_get_residuals(self._h, slot, _p(r)))
        return r

    def loss_param(self, slot, method, current=0.0):
        tau = C.c_double(current)
        _check(lib().eds_trk_loss_param(self._h, slot, int(method), C.cast(C.byref(tau), _dp)))
        return tau.value

    def residuals_and_loss(self, slot, method, current=0.0):
        """Tracker.cpp:223-233 in one call: (kf->residuals as the MAD selection leaves them, loss scale)."""
        r = np.zeros(self._N[slot])
        tau = C.c_double(current)
        _check(lib().eds_trk_residuals_and_loss(self._h, slot, int(method), _p(r), C.cast(C.byref(tau), _dp)))
        return r, tau.value

    def loss_param_batch(self, method, first=0, count=None):
        count = self.batch - first if count is None else count
        tau = np.zeros(count)
        _check(lib().eds_trk_loss_param_batch(self._h, first, count, int(method), _p(tau)))
        return tau

    def update_points(self, slot, delete_out_points=True):
        """Tracker::getCoord(delete_out_point): returns dict(coord, tracks, kept, mean_sq_flow)."""
        N = self._N[slot]
        coord, tracks = np.zeros((N, 2)), np.zeros((N, 2))
        kept = np.zeros(N, dtype=np.int32)
        n, flow = C.c_int32(0), C.c_double(0.0)
        _check(lib().eds_trk_update_points(self._h, slot, int(bool(delete_out_points)), _p(coord), _p(tracks),
                                           kept.ctypes.data_as(_ip), C.cast(C.byref(n), _ip), C.cast(C.byref(flow), _dp)))
        self._N[slot] = n.value
        return dict(coord=coord[:n.value], tracks=tracks[:n.value], kept=kept[:n.value], mean_sq_flow=flow.value)

    def update_points_batch(self, first=0, count=None, delete_out_points=True, want_points=True):
        """Tracker::getCoord(delete_out_point) for a range of slots in one call: list of dicts like update_points (coord / tracks /
        kept are None with want_points=False: only culling, counts and the mean squared flow)."""
        count = self.batch - first if count is None else count
        stride = max(self._N[first:first + count] + [1])
        n = np.zeros(count, dtype=np.int32); flow = np.zeros(count)
        if want_points:
            coord, tracks = np.zeros((count, stride, 2)), np.zeros((count, stride, 2))
            kept = np.zeros((count, stride), dtype=np.int32)
            _check(lib().eds_trk_update_points_batch(self._h, first, count, int(bool(delete_out_points)), stride, _p(coord), _p(tracks),
                                                     kept.ctypes.data_as(_ip), n.ctypes.data_as(_ip), _p(flow)))
        else:
            _check(lib().eds_trk_update_points_batch(self._h, first, count, int(bool(delete_out_points)), stride, None, None, None,
                                                     n.ctypes.data_as(_ip), _p(flow)))
        out = []
        for b in range(count):
            self._N[first + b] = int(n[b])
            out.append(dict(coord=coord[b, :n[b]] if want_points else None, tracks=tracks[b, :n[b]] if want_points else None,
                            kept=kept[b, :n[b]] if want_points else None, mean_sq_flow=float(flow[b]), n=int(n[b])))
        return out

    # -- KLT point trackers (include/eds_hip_klt.h) -------------------------------------------
    def _klt(self, fn, first, count, arg):
        count = self.batch - first if count is None else count
        stride = max(self._N[first:first + count] + [1])
        coord, tracks, flow = np.zeros((count, stride, 2)), np.zeros((count, stride, 2)), np.zeros((count, stride, 2))
        kept, n = np.zeros((count, stride), dtype=np.int32), np.zeros(count, dtype=np.int32)
        _check(fn(self._h, int(first), int(count), int(arg), stride, _p(coord), _p(tracks), _p(flow), kept.ctypes.data_as(_ip),
                  n.ctypes.data_as(_ip)))
        out = []
        for b in range(count):
            self._N[first + b] = int(n[b])
            out.append(dict(coord=coord[b, :n[b]], tracks=tracks[b, :n[b]], flow=flow[b, :n[b]], kept=kept[b, :n[b]], n=int(n[b])))
        return out

    def klt_track_points(self, first=0, count=None, patch_radius=7):
        """Tracker::trackPoints for slots first .. first + count - 1: getCoord(true), then the KLT flow of every kept point against the
        slot's event frame.  Returns per slot dict(coord, tracks, flow, kept, n) — tracks and flow as the device keeps them."""
        return self._klt(lib().eds_klt_track_points, first, count, patch_radius)

    def klt_track_points_pyr(self, first=0, count=None, num_level=3):
        """Tracker::trackPointsPyr; returns as klt_track_points (flow accumulates over calls until the next keyframe)."""
        return self._klt(lib().eds_klt_track_points_pyr, first, count, num_level)

    def klt_get(self, slot):
        """The device's kf->tracks and kf->flow of one slot: (N x 2, N x 2)."""
        N = self._N[slot]
        tracks, flow = np.zeros((N, 2)), np.zeros((N, 2))
        _check(lib().eds_klt_get(self._h, int(slot), _p(tracks), _p(flow)))
        return tracks, flow

    # -- epiline tracker (include/eds_hip_epiline.h) -------------------------------------------
    def epi_track_points(self, first=0, count=None, patch_radius=7, border_type=EPI_BORDER_REFLECT_101, border_value=255, erase=True):
        """Tracker::trackPointsAlongEpiline for slots first .. first + count - 1.  Returns per slot dict(ssd, ncc, scores) for every
        ORIGINAL point (int pixel pairs, the two fp32 scores), and dict(ef, kept, n) for the points the cull kept."""
        count = self.batch - first if count is None else count
        stride = max(self._N[first:first + count] + [1])
        ssd, ncc = np.zeros((count, stride, 2), dtype=np.int32), np.zeros((count, stride, 2), dtype=np.int32)
        scores, ef = np.zeros((count, stride, 2)), np.zeros((count, stride, 2))
        kept, n = np.zeros((count, stride), dtype=np.int32), np.zeros(count, dtype=np.int32)
        n0 = list(self._N[first:first + count])
        _check(lib().eds_epi_track_points(self._h, int(first), int(count), int(patch_radius), int(border_type), int(border_value),
                                          int(bool(erase)), stride, ssd.ctypes.data_as(_ip), ncc.ctypes.data_as(_ip), _p(scores), _p(ef),
                                          kept.ctypes.data_as(_ip), n.ctypes.data_as(_ip)))
        out = []
        for b in range(count):
            self._N[first + b] = int(n[b])
            out.append(dict(ssd=ssd[b, :n0[b]], ncc=ncc[b, :n0[b]], scores=scores[b, :n0[b]], ef=ef[b, :n[b]], kept=kept[b, :n[b]],
                            n=int(n[b])))
        return out

    def epi_get(self, slot):
        """the device ef plane of one slot, N x 2"""
        ef = np.zeros((self._N[slot], 2))
        _check(lib().eds_epi_get(self._h, int(slot), _p(ef)))
        return ef

    def epi_get_model(self, slot):
        """getModel(v, w, "bilinear", 0.5) at the slot's velocity and points, H x W fp64"""
        m = np.zeros((self.H, self.W))
        _check(lib().eds_epi_get_model(self._h, int(slot), _p(m)))
        return m

    def epi_depth_update(self, first=0, count=None, T_kf_ef=None, filter=DEPTH_VOGIATZIS):
        """DepthPoints::update(T_kf_ef, kf->coord, ef_coord) with ef_coord = the device ef plane; returns the summaries"""
        count = self.batch - first if count is None else count
        T = None if T_kf_ef is None else _f64(T_kf_ef).reshape(count, 7)
        out = (DepthSummary * count)()
        _check(lib().eds_epi_depth_update(self._h, int(first), int(count), _p(T), int(filter), out))
        return [o.as_dict() for o in out]

    # -- the keyframe's own point set (include/eds_hip_kfpoints.h) --------------------------------
    def _kfp_kept(self, first, count, kept, n):
        out = []
        for b in range(count):
            self._N[first + b] = int(n[b])
            out.append(dict(kept=kept[b, :n[b]].copy(), n=int(n[b])))
        return out

    def refine_points(self, first=0, count=None, event_diff=1.0, patch_radius=11, border_type=EPI_BORDER_REFLECT_101, border_value=255,
                      erase=True):
        """KeyFrame::pointsRefinement for slots first .. first + count - 1 on the frame each slot's solve reads.  Returns per slot
        dict(range, kept, n): max - min of every ORIGINAL point's window, and the kept points' original indices."""
        count = self.batch - first if count is None else count
        n0 = list(self._N[first:first + count])
        stride = max(n0 + [1])
        rng = np.zeros((count, stride))
        kept, n = np.zeros((count, stride), dtype=np.int32), np.zeros(count, dtype=np.int32)
        _check(lib().eds_kfp_refine_points(self._h, int(first), int(count), float(event_diff), int(patch_radius), int(border_type),
                                           int(border_value), int(bool(erase)), stride, _p(rng), kept.ctypes.data_as(_ip),
                                           n.ctypes.data_as(_ip)))
        out = self._kfp_kept(first, count, kept, n)
        for b in range(count):
            out[b]["range"] = rng[b, :n0[b]].copy()
        return out

    def clean_points(self, first=0, count=None, w_norm_thr=0.2):
        """KeyFrame::cleanPoints(w_norm_thr) on the slots' weight planes; per slot dict(kept, n)"""
        count = self.batch - first if count is None else count
        stride = max(self._N[first:first + count] + [1])
        kept, n = np.zeros((count, stride), dtype=np.int32), np.zeros(count, dtype=np.int32)
        _check(lib().eds_kfp_clean_points(self._h, int(first), int(count), float(w_norm_thr), stride, kept.ctypes.data_as(_ip),
                                          n.ctypes.data_as(_ip)))
        return self._kfp_kept(first, count, kept, n)

    def erase_points(self, which, first=0, count=None):
        """KeyFrame::erasePoint: `which` holds per slot either a boolean mask over its points or a list of indices (one such entry
        alone means one slot); per slot dict(kept, n)"""
        count = self.batch - first if count is None else count
        if count == 1 and not (isinstance(which, (list, tuple)) and len(which) == 1 and np.ndim(which[0]) == 1):
            which = [which]
        if len(which) != count:
            raise EdsError(ERR_INVALID, "one mask or index list per slot")
        stride = max(self._N[first:first + count] + [1])
        flags = np.zeros((count, stride), dtype=np.uint8)
        for b in range(count):
            w, N = np.asarray(which[b]), self._N[first + b]
            if w.dtype == np.bool_:
                if w.shape != (N,):
                    raise EdsError(ERR_INVALID, "an erase mask has one entry per point of its slot")
                flags[b, :N] = w
            else:
                w = w.astype(np.int64).ravel()
                if w.size and (w.min() < 0 or w.max() >= N):
                    raise EdsError(ERR_INVALID, "an erase index lies outside its slot's points")
                flags[b, w] = 1
        kept, n = np.zeros((count, stride), dtype=np.int32), np.zeros(count, dtype=np.int32)
        _check(lib().eds_kfp_erase_points(self._h, int(first), int(count), stride, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          kept.ctypes.data_as(_ip), n.ctypes.data_as(_ip)))
        return self._kfp_kept(first, count, kept, n)

    def point_counts(self, first=0, count=None):
        """(KeyFrame::num_points, coord.size()) per slot, two int arrays"""
        count = self.batch - first if count is None else count
        num, cur = np.zeros(count, dtype=np.int32), np.zeros(count, dtype=np.int32)
        _check(lib().eds_kfp_counts(self._h, int(first), int(count), num.ctypes.data_as(_ip), cur.ctypes.data_as(_ip)))
        return num, cur

    def project_depth_map(self, first=0, count=None, T=None, K=None, size=None):
        """getDepthMap() -> T_dst_src -> IDepthMap::fromPoints: the depth map the next keyframe's build_keyframe takes.  T: count x 7
        (p, q_xyzw) or None (each slot's state); K: count x 4 or None (the slot's own); size: (dst_H, dst_W) or None (the handle's).
        Returns per slot dict(xy, idp, src, n)."""
        count = self.batch - first if count is None else count
        stride = max(self._N[first:first + count] + [1])
        T = None if T is None else _f64(T).reshape(count, 7)
        K = None if K is None else _f64(K).reshape(count, 4)
        dH, dW = (0, 0) if size is None else (int(size[0]), int(size[1]))
        xy, idp = np.zeros((count, stride, 2)), np.zeros((count, stride))
        src, n = np.zeros((count, stride), dtype=np.int32), np.zeros(count, dtype=np.int32)
        _check(lib().eds_kfp_project_depth_map(self._h, int(first), int(count), _p(T), _p(K), dH, dW, stride, _p(xy), _p(idp),
                                               src.ctypes.data_as(_ip), n.ctypes.data_as(_ip)))
        return [dict(xy=xy[b, :n[b]].copy(), idp=idp[b, :n[b]].copy(), src=src[b, :n[b]].copy(), n=int(n[b])) for b in range(count)]

    # -- the keyframe switch for a range of slots (include/eds_hip_kfswitch.h) ----------------------
    def build_tree(self, maps):
        """``eds_kfs_build_tree``: the k-d tree's index array of every depth map.  `maps`: a list of m x 2 arrays (numpy: uploaded
        here), or a float64 device array count x S x 2 with a list of sizes, as ``(device_array, n)``.  Returns
        ``(list of int32 index arrays, on_host flags)``; on_host[b] is True where the map was ambiguous or beyond
        ``tree_capacity()`` and the host build made the array."""
        keep = None
        if isinstance(maps, tuple) and len(maps) == 2 and is_device_array(maps[0]):
            n = np.ascontiguousarray(maps[1], dtype=np.int32)
            count = int(n.shape[0])
            ptr, S, stride = _device_rows(maps[0], count, 2, "maps")
            if count and int(n.max()) > S:
                raise EdsError(ERR_INVALID, "a map has more points than its row holds")
        else:
            maps = [_f64(m).reshape(-1, 2) for m in maps]
            count = len(maps)
            n = np.array([m.shape[0] for m in maps], dtype=np.int32)
            stride = max(1, int(n.max()) if count else 1)
            t = np.zeros((max(count, 1), stride, 2))
            for b, m in enumerate(maps):
                t[b, :m.shape[0]] = m
            keep = DeviceArray.from_numpy(t)
            ptr = keep.ptr
        perm, on_host = np.zeros((max(count, 1), stride), dtype=np.int32), np.zeros(max(count, 1), dtype=np.uint8)
        _check(lib().eds_kfs_build_tree(self._h, count, n.ctypes.data_as(_ip), C.c_void_p(ptr or None), int(stride), perm.ctypes.data_as(_ip),
                                        on_host.ctypes.data_as(C.POINTER(C.c_uint8))))
        del keep
        return [perm[b, :n[b]].copy() for b in range(count)], on_host[:count].astype(bool)

    def build_keyframes(self, images, K, first=0, depth=None, depth_idp=None, depth_n=None, src_first=None, T=None, K_dst=None, method=KF_MEDIAN,
                        num_points=0, cell=20, min_depth=1.0, max_depth=3.0, weight_threshold=0.7, sobel_ksize=3, vectors=True, check=True):
        """``eds_kfs_build_keyframes[_dev]``: KeyFrame::create for slots first .. first + count - 1 in one call.

        images: count grey H x W images — a numpy array count x H x W (or a list of H x W arrays) of uint8 / float32 / float64, or
        anything with ``__cuda_array_interface__`` of that shape (strided frames and rows are fine).  K: count x 4.
        depth: None (the constant initial depth); ``"slots"`` — each map is the projection of slot ``src_first + b`` (default: in place)
        by T (count x 7, None: the solved state) and K_dst (count x 4, None: the slot's own); a list of m x 2 arrays (None or empty: that
        slot has no map) with `depth_idp` a list of m-vectors; or device arrays count x S x 2 / count x S with `depth_n` sizes.
        Returns per slot dict(status, n, tree_on_host[, coord, norm_coord, grad, idp, weights]).  check: raise EdsError at the first
        failing slot's code after all slots were tried (False: look at status)."""
        if is_device_array(images):
            ptr, count, ty, fstride, rstride = _kfs_device_images(images, self.H, self.W)
            host_imgs = None
        else:
            host_imgs = [np.ascontiguousarray(im) for im in images]
            count = len(host_imgs)
            dts = {im.dtype for im in host_imgs}
            if count < 1 or len(dts) != 1 or any(im.shape != (self.H, self.W) for im in host_imgs):
                raise EdsError(ERR_INVALID, "images must be count x H x W of one dtype")
            dt = dts.pop()
            ty = IMG_U8 if dt == np.uint8 else (IMG_F32 if dt == np.float32 else IMG_F64)
            if ty == IMG_F64:
                host_imgs = [np.ascontiguousarray(im, dtype=np.float64) for im in host_imgs]
        K = None if K is None else _f64(K).reshape(count, 4)          # None: the source slots' own (depth="slots" only)
        sel = KfSelect()
        lib().eds_kf_select_default(C.byref(sel))
        sel.method, sel.cell, sel.num_points, sel.sobel_ksize = int(method), int(cell), int(num_points), int(sobel_ksize)
        sel.min_depth, sel.max_depth, sel.weight_threshold = float(min_depth), float(max_depth), float(weight_threshold)
        d, keep = KfsDepth(), []
        if depth is None:
            d.source = KFS_DEPTH_NONE
        elif isinstance(depth, str):
            if depth != "slots":
                raise EdsError(ERR_INVALID, 'depth is None, "slots", a list of maps or device arrays')
            d.source, d.src_first = KFS_DEPTH_SLOTS, int(first if src_first is None else src_first)
            if T is not None:
                keep.append(_f64(T).reshape(count, 7)); d.T7 = keep[-1].ctypes.data
            if K_dst is not None:
                keep.append(_f64(K_dst).reshape(count, 4)); d.K_dst = keep[-1].ctypes.data
        elif is_device_array(depth):
            n = np.ascontiguousarray(depth_n, dtype=np.int32).reshape(count)
            pxy, S, stride = _device_rows(depth, count, 2, "depth")
            pidp, S2, stride2 = _device_rows(depth_idp, count, 1, "depth_idp")
            if stride2 != stride or int(n.max()) > min(S, S2):
                raise EdsError(ERR_INVALID, "depth and depth_idp have different strides, or a map has more points than its row holds")
            keep.append(n)
            d.source, d.n, d.depth_xy, d.depth_idp, d.stride = KFS_DEPTH_DEVICE, n.ctypes.data, pxy, pidp, stride
        else:
            maps = [np.zeros((0, 2)) if m is None else _f64(m).reshape(-1, 2) for m in depth]
            idps = [np.zeros(0) if m is None else _f64(m).reshape(-1) for m in (depth_idp if depth_idp is not None else [None] * count)]
            if len(maps) != count or len(idps) != count or any(a.shape[0] != b.shape[0] for a, b in zip(maps, idps)):
                raise EdsError(ERR_INVALID, "one depth map and one inverse-depth vector of the same length per slot")
            n = np.array([m.shape[0] for m in maps], dtype=np.int32)
            stride = max(1, int(n.max()))
            txy, tidp = np.zeros((count, stride, 2)), np.zeros((count, stride))
            for b in range(count):
                txy[b, :n[b]], tidp[b, :n[b]] = maps[b], idps[b]
            keep += [n, txy, tidp]
            d.source, d.n, d.depth_xy, d.depth_idp, d.stride = KFS_DEPTH_HOST, n.ctypes.data, txy.ctypes.data, tidp.ctypes.data, stride
        o = KfsOut()
        n_points, status, on_host = np.full(count, -1, dtype=np.int32), np.zeros(count, dtype=np.int32), np.zeros(count, dtype=np.uint8)
        o.n_points, o.status, o.tree_on_host = n_points.ctypes.data, status.ctypes.data, on_host.ctypes.data
        vec = {}
        if vectors:
            S = self.max_points
            vec = dict(coord=np.zeros((count, S, 2)), norm_coord=np.zeros((count, S, 2)), grad=np.zeros((count, S, 2)), idp=np.zeros((count, S)),
                       weights=np.zeros((count, S)))
            o.stride = S
            o.coord_xy, o.norm_xy, o.grad_xy = vec["coord"].ctypes.data, vec["norm_coord"].ctypes.data, vec["grad"].ctypes.data
            o.idp, o.weights = vec["idp"].ctypes.data, vec["weights"].ctypes.data
        if host_imgs is None:
            rc = lib().eds_kfs_build_keyframes_dev(self._h, int(first), count, ty, C.c_void_p(ptr or None), fstride, rstride, C.byref(sel), _p(K),
                                                   C.byref(d), C.byref(o))
        else:
            ptrs = (C.c_void_p * count)(*[im.ctypes.data for im in host_imgs])
            rc = lib().eds_kfs_build_keyframes(self._h, int(first), count, ty, ptrs, C.byref(sel), _p(K), C.byref(d), C.byref(o))
        if rc != EDS_OK and not status.any():       # refused as a whole: nothing was tried
            _check(rc)
        out = []
        for b in range(count):
            r = dict(status=int(status[b]), n=int(n_points[b]), tree_on_host=bool(on_host[b]))
            if status[b] == EDS_OK:
                self._N[first + b] = r["n"]
                for k_, v in vec.items():
                    r[k_] = v[b, :r["n"]].copy()
            out.append(r)
        if check:
            _check(rc)
        return out

    # -- inverse-depth filter (include/eds_hip_depth.h) -----------------------------------------
    def depth_init(self, first=0, count=None, source=DEPTH_INIT_CONSTANT, idp=None, min_depth=1.0, max_depth=3.0, threshold=100.0,
                   init_a=2.0, init_b=5.0):
        """DepthPoints::init for slots first .. first + count - 1.  idp (DEPTH_INIT_HOST): one row of inverse depths per slot
        (count x stride array, or a list of per-slot vectors)."""
        count = self.batch - first if count is None else count
        prm = DepthParams(float(min_depth), float(max_depth), float(threshold), float(init_a), float(init_b))
        t, stride = (None, 1) if idp is None else _rows(idp, count, 1)
        _check(lib().eds_depth_init(self._h, int(first), int(count), C.byref(prm), int(source), _p(t), int(stride)))

    def depth_update(self, first=0, count=None, coords=DEPTH_REPROJECT, xy=None, kf_xy=None, T_kf_ef=None, filter=DEPTH_VOGIATZIS):
        """DepthPoints::update for slots first .. first + count - 1.  xy / kf_xy: per slot N x 2 pixels (a count x stride x 2 array or a
        list of N x 2 arrays); T_kf_ef: count x 7 (p, q_xyzw) or None (the inverse of each slot's pose).  Returns the summaries."""
        count = self.batch - first if count is None else count
        stride = 1
        a = b = None
        if xy is not None:
            a, stride = _rows(xy, count, 2)
        if kf_xy is not None:
            b, stride2 = _rows(kf_xy, count, 2)
            if a is not None and stride2 != stride:
                raise EdsError(ERR_INVALID, "xy and kf_xy have different strides")
            stride = stride2
        T = None if T_kf_ef is None else _f64(T_kf_ef).reshape(count, 7)
        out = (DepthSummary * count)()
        _check(lib().eds_depth_update(self._h, int(first), int(count), int(coords), _p(a), _p(b), int(stride), _p(T), int(filter), out))
        return [o.as_dict() for o in out]

    def depth_get(self, slot):
        """the seeds of a slot: (N x 4 [mu, sigma2, a, b], N converged flags)"""
        N = self._N[slot]
        seeds, conv = np.zeros((N, 4)), np.zeros(N, dtype=np.uint8)
        _check(lib().eds_depth_get(self._h, int(slot), _p(seeds), conv.ctypes.data_as(C.POINTER(C.c_uint8))))
        return seeds, conv.astype(bool)

    def depth_set(self, slot, seeds):
        s = _f64(seeds)
        if s.shape != (self._N[slot], 4):
            raise EdsError(ERR_INVALID, "seeds must be N x 4")
        _check(lib().eds_depth_set(self._h, int(slot), _p(s)))

    def depth_get_idepth(self, slot):
        mu = np.zeros(self._N[slot])
        _check(lib().eds_depth_get_idepth(self._h, int(slot), _p(mu)))
        return mu

    def depth_stats(self, first=0, count=None):
        """count x 4: mean, "std_dev" (the n-1 variance), median (n/2-th), "third_q" (n/3-th) of mu"""
        count = self.batch - first if count is None else count
        out = np.zeros((count, 4))
        _check(lib().eds_depth_stats(self._h, int(first), int(count), _p(out)))
        return out

    # -- keyframe set-up on the device ------------------------------------------------------
    def build_keyframe(self, slot, img, K, method=KF_MEDIAN, num_points=0, cell=20, depth_xy=None, depth_idp=None,
                       min_depth=1.0, max_depth=3.0, weight_threshold=0.7, sobel_ksize=3):
        """KeyFrame::create's tracker-facing part on the device; returns dict(coord, norm_coord, grad, idp, weights)."""
        img = np.ascontiguousarray(img)
        if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)):
            raise EdsError(ERR_INVALID, "image must be H x W (grey) or H x W x 3 (RGB)")
        channels = 1 if img.ndim == 2 else int(img.shape[2])
        img_H, img_W = int(img.shape[0]), int(img.shape[1])      # != (self.H, self.W): out_scale != 1, resized on the device
        if img.dtype == np.uint8:
            ty = IMG_U8
        elif img.dtype == np.float32:
            ty = IMG_F32
        else:
            ty, img = IMG_F64, np.ascontiguousarray(img, dtype=np.float64)
        sel = KfSelect()
        lib().eds_kf_select_default(C.byref(sel))
        sel.method, sel.cell, sel.num_points, sel.sobel_ksize = int(method), int(cell), int(num_points), int(sobel_ksize)
        sel.min_depth, sel.max_depth, sel.weight_threshold = float(min_depth), float(max_depth), float(weight_threshold)
        nd = 0 if depth_xy is None else len(depth_xy)
        dxy = _f64(depth_xy) if nd else None
        didp = _f64(depth_idp) if nd else None
        n = C.c_int32(0)
        fx, fy, cx, cy = [float(k) for k in K]
        if channels == 1 and (img_H, img_W) == (self.H, self.W):
            _check(lib().eds_trk_build_keyframe(self._h, slot, ty, img.ctypes.data_as(C.c_void_p), C.byref(sel), nd,
                                                _p(dxy) if nd else None, _p(didp) if nd else None, fx, fy, cx, cy,
                                                C.cast(C.byref(n), _ip)))
        else:
            _check(lib().eds_trk_build_keyframe_image(self._h, slot, ty, img.ctypes.data_as(C.c_void_p), img_H, img_W, channels,
                                                      C.byref(sel), nd, _p(dxy) if nd else None, _p(didp) if nd else None,
                                                      fx, fy, cx, cy, C.cast(C.byref(n), _ip)))
        N = n.value
        self._N[slot] = N
        out = dict(coord=np.zeros((N, 2)), norm_coord=np.zeros((N, 2)), grad=np.zeros((N, 2)), idp=np.zeros(N), weights=np.zeros(N))
        _check(lib().eds_trk_get_keyframe_points(self._h, slot, _p(out["coord"]), _p(out["norm_coord"]), _p(out["grad"]),
                                                 _p(out["idp"]), _p(out["weights"])))
        return out

    # -- measurement ---------------------------------------------------------------------
    def timer_start(self):
        _check(lib().eds_trk_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float(0.0)
        _check(lib().eds_trk_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def prepare_frames(self, first=0, count=None, force=False) -> float:
        """Converts the (stale, or with force all) frames of the range to the strip layout now; returns the device time in ms."""
        count = self.batch - first if count is None else count
        ms = C.c_float(0.0)
        _check(lib().eds_trk_prepare_frames(self._h, int(first), int(count), int(bool(force)), C.byref(ms)))
        return ms.value

    def set_knob(self, name: str, value=None) -> None:
        """One tuning knob of THIS handle (``eds_trk_set_knob``): same names and values as the environment variables the handle read at
        creation; ``None`` / ``""`` restores the default."""
        _check(lib().eds_trk_set_knob(self._h, name.encode(), None if value is None else str(value).encode()))

    def strips_info(self) -> dict:
        b, ph, un = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        _check(lib().eds_trk_get_strips_info(self._h, C.byref(b), C.byref(ph), C.byref(un)))
        return dict(bytes=int(b.value), row_phases=int(ph.value), unavailable=bool(un.value))

    def last_launch(self) -> dict:
        li = LaunchInfo()
        _check(lib().eds_trk_last_launch(self._h, C.byref(li)))
        d = {k: getattr(li, k) for k, _ in li._fields_}
        d["kernel"] = li.kernel.decode()
        return d

    def bench_live(self, slot, p0, q0, v0, level=0, idp=None, frame=None, method=-1, reps=50) -> dict:
        """``eds_trk_bench_live``: the live sequence timed inside the library (medians, microseconds)."""
        p0, q0, v0 = _f64(p0), _f64(q0), _f64(v0)
        idp = None if idp is None else _f64(idp)
        frame = None if frame is None else _f64(frame)
        out = np.zeros(6)
        _check(lib().eds_trk_bench_live(self._h, int(slot), int(level), None if idp is None else _p(idp), None if frame is None else _p(frame),
                                        _p(p0), _p(q0), _p(v0), int(method), int(reps), _p(out)))
        return dict(zip(("total_us", "set_idepth_us", "set_event_frame_us", "optimize_us", "residuals_and_loss_us", "kernel_us"), out.tolist()))

    def bench_batch(self, P, Q, V, first=0, level=0, reps=50) -> dict:
        """``eds_trk_bench_batch``: reps x {set_states; optimize_batch_wait} timed inside the library (medians + the slowest step, microseconds)."""
        P, Q, V = _f64(P), _f64(Q), _f64(V)
        out = np.zeros(5)
        _check(lib().eds_trk_bench_batch(self._h, int(level), int(first), int(P.shape[0]), _p(P), _p(Q), _p(V), int(reps), _p(out)))
        return dict(zip(("step_us", "set_states_us", "solve_us", "kernel_us", "slowest_step_us"), out.tolist()))

    def bench_eval(self, first, count, ncols=6, with_reduction=False, reps=20) -> float:
        ms = C.c_float(0.0)
        _check(lib().eds_trk_bench_eval(self._h, first, count, ncols, int(with_reduction), reps, C.byref(ms)))
        return ms.value


    def bench_kernel_cold(self, first, count, ncols=6, which=0, reps=10) -> float:
        """One streaming kernel (which: 0 residual/Jacobian, 1 reduction) timed cold — 1 GiB streamed through the caches in front of
        every repetition; mean ms per launch (HIP events on the handle's stream)."""
        ms = C.c_float(0.0)
        _check(lib().eds_trk_bench_kernel_cold(self._h, first, count, ncols, int(which), reps, C.byref(ms)))
        return ms.value

    def hbm_probe(self, nbytes=1 << 30, reps=10) -> dict:
        """What the box's HBM streams through the library's own plain kernel: read-only pass and copy (read + write counted), GB/s."""
        r, c = C.c_float(0.0), C.c_float(0.0)
        _check(lib().eds_trk_hbm_probe(self._h, int(nbytes), reps, C.byref(r), C.byref(c)))
        return {"read_GBps": r.value, "copy_GBps": c.value, "bytes": int(nbytes), "reps": reps}


def kernel_instances(family: int):
    """The compiled instantiations of eds_fused6_kernel (family 0: S, P, T, Q, K, G) / eds_fused12_kernel (1: S, T, CAP, NC, K, Q)."""
    L = lib()
    n = L.eds_trk_kernel_instances(int(family), -1, None)
    out = []
    for i in range(max(n, 0)):
        a = (C.c_int32 * 6)()
        L.eds_trk_kernel_instances(int(family), i, a)
        out.append(tuple(int(x) for x in a))
    return out


class Pyramid:
    """RAII wrapper of ``eds_pyr*``: coarse-to-fine tracking of one alignment on an image pyramid (BASELINE.json configs[3])."""

    def __init__(self, cfg: Cfg, max_points, H: int, W: int, batch: int = 1):
        self.levels = len(max_points)
        self.H, self.W, self.batch = int(H), int(W), int(batch)
        mp = np.ascontiguousarray(max_points, dtype=np.int32)
        self._h = C.c_void_p()
        self._N = [0] * self.levels
        _check(lib().eds_pyr_create_batch(C.byref(cfg), self.batch, self.levels, mp.ctypes.data_as(_ip), self.H, self.W, C.byref(self._h)))

    # -- batched pyramids (batch > 1): the same calls per pyramid (slot), one launch per level for all of them ----------------
    def set_keyframe_slot(self, slot, level, norm_coord, grad, idp, weights, fx, fy, cx, cy):
        nc, g, d, w = _f64(norm_coord), _f64(grad), _f64(idp), _f64(weights)
        self._N[level] = max(self._N[level], int(d.shape[0]))
        _check(lib().eds_pyr_set_keyframe_slot(self._h, int(slot), int(level), int(d.shape[0]), _p(nc), _p(g), _p(d), _p(w), fx, fy, cx, cy))

    def set_event_frame_slot(self, slot, frame):
        f = _f64(frame)
        assert f.size == self.H * self.W
        _check(lib().eds_pyr_set_event_frame_slot(self._h, int(slot), _p(f)))

    def optimize_batch(self, P, Q, V, first=0, want_infos=True):
        """P, Q, V: count x 3 / 4 / 6 start states of pyramids [first, first + count).  Returns (P, Q, V, infos[level][k])."""
        P, Q, V = _f64(P).copy(), _f64(Q).copy(), _f64(V).copy()
        count = P.shape[0]
        infos = (Info * (self.levels * count))() if want_infos else None
        _check(lib().eds_pyr_optimize_batch(self._h, int(first), count, _p(P), _p(Q), _p(V), infos))
        out = [[infos[l * count + k].as_dict() for k in range(count)] for l in range(self.levels)] if want_infos else None
        return P, Q, V, out

    def close(self):
        if self._h:
            lib().eds_pyr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_config(self, cfg: Cfg):
        _check(lib().eds_pyr_set_config(self._h, C.byref(cfg)))

    @staticmethod
    def level_intrinsics(level, fx, fy, cx, cy):
        K = np.zeros(4)
        _check(lib().eds_pyr_level_intrinsics(int(level), fx, fy, cx, cy, _p(K)))
        return K

    def set_keyframe(self, level, norm_coord, grad, idp, weights, fx, fy, cx, cy):
        nc, g, d, w = _f64(norm_coord), _f64(grad), _f64(idp), _f64(weights)
        self._N[level] = int(d.shape[0])
        _check(lib().eds_pyr_set_keyframe(self._h, int(level), self._N[level], _p(nc), _p(g), _p(d), _p(w), fx, fy, cx, cy))

    def set_event_frame(self, frame):
        f = _f64(frame)
        assert f.size == self.H * self.W
        _check(lib().eds_pyr_set_event_frame(self._h, _p(f)))

    def build_event_frame(self, x, y, polarity, blur_sigma=0.5, use_exp_weights=True):
        x = np.ascontiguousarray(x, dtype=np.uint16); y = np.ascontiguousarray(y, dtype=np.uint16)
        pol = np.ascontiguousarray(polarity, dtype=np.uint8)
        norm = C.c_double(0.0)
        _check(lib().eds_pyr_build_event_frame(self._h, int(x.shape[0]), x.ctypes.data_as(C.POINTER(C.c_uint16)),
                                               y.ctypes.data_as(C.POINTER(C.c_uint16)), pol.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               float(blur_sigma), int(bool(use_exp_weights)), C.cast(C.byref(norm), _dp)))
        return norm.value

    def level_size(self, level):
        h, w = C.c_int32(0), C.c_int32(0)
        _check(lib().eds_pyr_level_size(self._h, int(level), C.byref(h), C.byref(w)))
        return h.value, w.value

    def level_frame(self, level):
        h, w = self.level_size(level)
        out = np.zeros((h, w))
        _check(lib().eds_pyr_get_level_frame(self._h, int(level), _p(out)))
        return out

    def optimize(self, p, q, v):
        """One call, coarsest level first.  Returns (p, q, v, [info per level, finest first])."""
        p, q, v = _f64(p).copy(), _f64(q).copy(), _f64(v).copy()
        infos = (Info * self.levels)()
        _check(lib().eds_pyr_optimize(self._h, _p(p), _p(q), _p(v), infos))
        return p, q, v, [infos[l].as_dict() for l in range(self.levels)]

    def residuals(self, level):
        r = np.zeros(self._N[level])
        _check(lib().eds_pyr_get_residuals(self._h, int(level), _p(r)))
        return r


def device_count() -> int:
    return int(lib().eds_device_count())
