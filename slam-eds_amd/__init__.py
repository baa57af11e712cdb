"""MI355X-native event-to-model photometric tracker for EDS (uzh-rpg/slam-eds hot path).

The directory name contains a hyphen, so load it with
``importlib.import_module("slam-eds_amd")`` (or ``import slam_eds_amd`` — the
alias module at the repo root).  Sub-modules:

* ``synth``   — deterministic synthetic workloads (numpy only)
* ``capi``    — ctypes binding of the C-ABI library ``csrc/libeds_hip.so``
* ``tracker`` — Python mirror of ``eds::tracking::Tracker`` (reference Tracker.hpp:36-114)
* ``batch``   — batched / multi-GPU alignment driver (one process per GPU, RCCL gather)
* ``depth``   — Python mirror of ``eds::mapping::DepthPoints`` whose seeds live on the device (include/eds_hip_depth.h)
* ``immature`` — DSO's immature points traced along epipolar lines on the device (include/eds_hip_immature.h)
* ``coarse``  — DSO's coarse image tracker for the pose of every new image frame, on the device (include/eds_hip_coarse.h)
* ``select``  — DSO's pixel selector: which pixels of a keyframe become immature points, on the device (include/eds_hip_select.h)
* ``window``  — the window optimiser's linearize, applyRes and per-point Hessian sums on the device (include/eds_hip_window.h)
* ``map``     — the map as a point cloud and as the next tracker keyframe's depth maps, on the device (include/eds_hip_map.h)
"""
__version__ = "0.1.0"
