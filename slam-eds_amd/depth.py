"""Python mirror of ``eds::mapping::DepthPoints`` (reference src/mapping/DepthPoints.{hpp,cpp}) whose seeds live on the device.

A ``DepthPoints`` is bound to one slot of a ``capi.Handle``: the seeds ``[mu, sigma2, a, b]`` stay in HBM next to the slot's point
planes (include/eds_hip_depth.h), every call that changes ``mu`` also refreshes the slot's inverse-depth plane and Gram matrices, so
``Handle.optimize`` on that slot solves with the filtered depths without an upload.  Member names are the reference's.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .tracker import _R_to_quat

VOGIATZIS, GAUSS = capi.DEPTH_VOGIATZIS, capi.DEPTH_GAUSS


def _pose7(T_kf_ef):
    """4 x 4 matrix or (p, q_xyzw) -> p[3] q[4] (None: the inverse of the slot's pose, as the device takes it)"""
    if T_kf_ef is None:
        return None
    if isinstance(T_kf_ef, (tuple, list)) and len(T_kf_ef) == 2:
        p, q = T_kf_ef
        return np.concatenate([np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)])
    T = np.asarray(T_kf_ef, dtype=np.float64)
    return np.concatenate([T[:3, 3], _R_to_quat(T[:3, :3])])


class DepthPoints:
    px_noise = 3.0

    def __init__(self, handle: "capi.Handle", slot: int = 0):
        self.handle, self.slot = handle, int(slot)
        self.mu_range = float("nan")
        self.convergence_sigma2_thresh = float("nan")
        self.K_ = np.full((3, 3), np.nan)

    def _check_K(self, K):
        K = np.asarray(K, dtype=np.float64)
        self.K_ = K.copy()
        self.px_error_angle = float(np.arctan(self.px_noise / (2.0 * K[0, 0])) + np.arctan(self.px_noise / (2.0 * K[1, 1])))

    def init(self, K, num_points_or_inv_depth, min_depth, max_depth, threshold=100.0, init_a=2.0, init_b=5.0):
        """Both overloads (DepthPoints.cpp:59-99): an int -> mu = 1/((max-min)/2), sigma2 = mu_range^2; a vector of inverse depths ->
        mu = idp, sigma2 = mu_range^2/36.  The string "plane" seeds from the slot's fp32 inverse-depth plane (narrowed values).
        The number of seeds is the slot's point count; K is recorded for the accessors (the device uses the keyframe's)."""
        self._check_K(K)
        h, n = self.handle, self.handle._N[self.slot]
        kw = dict(min_depth=min_depth, max_depth=max_depth, threshold=threshold, init_a=init_a, init_b=init_b)
        if isinstance(num_points_or_inv_depth, str):
            if num_points_or_inv_depth != "plane":
                raise ValueError("init source must be a count, a vector or 'plane'")
            h.depth_init(self.slot, 1, capi.DEPTH_INIT_PLANE, **kw)
        elif np.isscalar(num_points_or_inv_depth):
            if int(num_points_or_inv_depth) != n:
                raise capi.EdsError(capi.ERR_INVALID, f"the slot holds {n} points, not {num_points_or_inv_depth}")
            h.depth_init(self.slot, 1, capi.DEPTH_INIT_CONSTANT, **kw)
        else:
            idp = np.asarray(num_points_or_inv_depth, dtype=np.float64)
            if idp.shape != (n,):
                raise capi.EdsError(capi.ERR_INVALID, f"the slot holds {n} points, not {idp.shape}")
            h.depth_init(self.slot, 1, capi.DEPTH_INIT_HOST, idp=idp[None], **kw)
        self.mu_range = float(max_depth - min_depth)
        self.convergence_sigma2_thresh = float(threshold)

    def update(self, T_kf_ef=None, kf_coord=None, tracks_or_ef_coord=None, filter=VOGIATZIS, ef_coord=False):
        """update(T_kf_ef, kf_coord, tracks) (DepthPoints.cpp:137-178), or with ef_coord=True the ef_coord overload (:101-135).
        kf_coord None: the keyframe pixels the slot holds; tracks None: getCoord's tracks at the slot's pose, on the device.
        Returns the summary of the update."""
        if tracks_or_ef_coord is None:
            coords = capi.DEPTH_REPROJECT
        else:
            coords = capi.DEPTH_EF_COORD if ef_coord else capi.DEPTH_TRACKS
        T = _pose7(T_kf_ef)
        return self.handle.depth_update(self.slot, 1, coords, xy=None if tracks_or_ef_coord is None else np.asarray(tracks_or_ef_coord),
                                        kf_xy=None if kf_coord is None else np.asarray(kf_coord),
                                        T_kf_ef=None if T is None else T[None], filter=filter)[0]

    def getIDepth(self):
        return self.handle.depth_get_idepth(self.slot)

    def meanIDepth(self):
        """(mean, "st_dev") — the second is the n-1 variance, as mean_std_vector returns it (Utils.hpp:272-290)"""
        s = self.handle.depth_stats(self.slot, 1)[0]
        return float(s[0]), float(s[1])

    def medianIDepth(self):
        """(median, "third_q") — the nth_element at n/2 and at n/3 (DepthPoints.cpp:255-260)"""
        s = self.handle.depth_stats(self.slot, 1)[0]
        return float(s[2]), float(s[3])

    def isConverged(self):
        return self.handle.depth_get(self.slot)[1]

    def depthRange(self):
        return self.mu_range

    def K(self):
        return self.K_

    def size(self):
        return self.handle._N[self.slot]

    def __len__(self):
        return self.size()

    def empty(self):
        return self.size() == 0

    def data(self):
        """N x 4 [mu, sigma2, a, b]"""
        return self.handle.depth_get(self.slot)[0]

    def __getitem__(self, index):
        if not 0 <= index < self.size():
            raise IndexError("index out of bound")          # the reference prints and exits (DepthPoints.cpp:266-270)
        return self.data()[index]

    def __setitem__(self, index, value):
        if not 0 <= index < self.size():
            raise IndexError("index out of bound")
        d = self.data()
        d[index] = np.asarray(value, dtype=np.float64)
        self.handle.depth_set(self.slot, d)
