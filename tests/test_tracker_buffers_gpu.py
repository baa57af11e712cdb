"""The tracker handle's lazily grown buffers (one owner, one regrow helper).  For every buffer that a call allocates on demand,
one handle makes the call small and then large enough to force the regrow, a second handle makes only the large call and so allocates at
once; the large call's outputs agree bit for bit.  A regrow that left a stale carved pointer or a stale capacity behind would show here.
Both handles then solve the same batch to the same bits and are destroyed.  B = 3 slots, 48 x 64 frames, 200 points: every call takes the
argument shapes of its own module's tests, nothing is out of range.

The event-frame calls vote with unit weights (use_exp_weights = False).  The votes are atomic additions in an order the hardware chooses;
with unit weights every addend is +-1 or, under the undistortion map, +-a product of two fractions of fp32 coordinates that the map below
keeps above 4 (each a multiple of 2^-21, the product of 2^-42, a pixel's sum below 2^6), so every partial sum is exact in fp64 and the image
does not depend on that order.  With the window weights exp(..) it would, in its last
bits, on one handle called twice as well: that is no property of a buffer.  The frames are small enough (at most 48 workgroups a level)
that each of the 64 sum-of-squares accumulators of a level receives one addend."""
import importlib

import numpy as np
import pytest

import intrinsics_cases as ic
import kdbuild_cases as kc
import map_cases as mc

pytestmark = pytest.mark.gpu

B, H, W, N = 3, 48, 64, 200
AOS = np.dtype([("ts", np.int64), ("x", np.uint16), ("y", np.uint16), ("polarity", np.uint8)], align=True)


def _differ(a, b, where=""):
    """the leaves of two outputs (through dicts, lists and tuples) that are not the same bits, each with how far apart they are"""
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        return [d for k in a for d in _differ(a[k], b[k], f"{where}.{k}")]
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b):
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in _differ(x, y, f"{where}[{i}]")]
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return [f"{where}: {a.dtype}{a.shape} against {b.dtype}{b.shape}"]
    if a.tobytes() == b.tobytes():
        return []
    return [f"{where}: {int((a != b).sum())} of {a.size} differ, by at most {np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))):.3e}"]


def _events(seed, n, sH=H, sW=W):
    rng = np.random.default_rng([0x6576, seed])
    return rng.integers(0, sW, n).astype(np.uint16), rng.integers(0, sH, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8)


def _aos(seed, n):
    ev = np.zeros(n, dtype=AOS)
    ev["x"], ev["y"], ev["polarity"] = _events(seed, n)
    ev["ts"] = np.arange(n)
    return ev


def _lut(sH, sW):
    """a mild distortion of the sensor's pixel grid towards its centre: every event stays on the sensor"""
    yy, xx = np.mgrid[0:sH, 0:sW].astype(np.float64)
    r2 = ((xx - sW / 2) / sW) ** 2 + ((yy - sH / 2) / sH) ** 2
    return (xx - 0.8 * r2 * (xx - sW / 2)).astype(np.float32), (yy - 0.8 * r2 * (yy - sH / 2)).astype(np.float32)


def _map(m):
    """a depth map of exactly m points at real-valued pixels (no two share a coordinate: the device builds its k-d tree); (xy, idp)"""
    rng = np.random.default_rng([0x6D70, m])
    return np.column_stack([rng.uniform(0, W - 1, m), rng.uniform(0, H - 1, m)]), rng.uniform(0.3, 1.0, m)


def _frames(h, count=B):
    return [h.get_event_frame(s) for s in range(count)]


@pytest.fixture(scope="module")
def world(synth):
    """the inputs both handles share; nothing below changes them"""
    als = [synth.make_alignment(900 + b, H=H, W=W, N=N, margin=4) for b in range(B)]
    rng = np.random.default_rng(22)
    T7 = np.stack([np.concatenate([rng.normal(0, 0.01, 3), ic.QS()]) for _ in range(B)])
    K = np.array([[als[b].fx, als[b].fy, als[b].cx, als[b].cy] for b in range(B)])
    maps = {m: _map(m) for m in (40, 50, 150, 170, 190, 500)}
    return dict(als=als, T7=T7, K=K, maps=maps, imgs=[kc.image(70 + b, H, W) for b in range(B)],
                T_w_kf=np.stack([mc.random_pose(rng) for _ in range(B)]))


def _prepare(h, w):
    """every slot's keyframe, frame and start state as at the beginning: what a step's small call changed is put back"""
    h.set_undistort_map()
    for b, al in enumerate(w["als"]):
        h.set_alignment(b, al)


def _steps(w):
    """(name, small call, large call) per lazily grown buffer; each call returns everything that reads the buffer back"""
    mp = importlib.import_module("slam-eds_amd.map")
    capi = importlib.import_module("slam-eds_amd.capi")
    als, T7, K, maps, imgs = w["als"], w["T7"], w["K"], w["maps"], w["imgs"]
    near = [al.coord + 0.3 for al in als]
    sel = dict(cell=8, method=capi.KF_MAX, num_points=192)         # 48 cells, the 4 strongest gradients of each: 192 candidates <= max_points

    def levels(n_levels, n_events):
        return lambda h: (h.build_event_frames(0, n_levels, *_events(1, n_events), use_exp_weights=False), _frames(h, n_levels))

    def levels_aos(n_levels, n_events):
        return lambda h: (h.build_event_frames_aos(0, n_levels, _aos(2, n_events), use_exp_weights=False), _frames(h, n_levels))

    def batch(count):
        return lambda h: (h.build_event_frame_batch(0, [_events(10 + b, 700 + 300 * b) for b in range(count)], use_exp_weights=False), _frames(h, count))

    def lut(sH, sW):
        def call(h):
            h.set_undistort_map_sized(*_lut(sH, sW), (sH, sW))
            return h.build_event_frames(0, 2, *_events(3, 3000, sH, sW), sensor_size=(sH, sW), use_exp_weights=False), _frames(h, 2)
        return call

    def upload(count):
        def call(h):
            h.set_event_frames(0, [als[(b + 1) % B].frame for b in range(count)])
            return _frames(h, count)
        return call

    def depth(count):
        def call(h):
            h.depth_init(0, count)
            a = h.depth_update(0, count, capi.DEPTH_EF_COORD, xy=near[:count])          # host coordinates: the filter's input buffer
            b = h.depth_update(0, count)
            return a, b, [h.depth_get(s) for s in range(count)], h.depth_stats(0, count)
        return call

    def keyframes(count, sizes):
        def call(h):
            trees = h.build_tree([maps[m][0] for m in sizes])
            outs = h.build_keyframes(np.stack(imgs[:count]), K[:count], depth=[maps[m][0] for m in sizes], depth_idp=[maps[m][1] for m in sizes],
                                     check=False, **sel)
            assert all(o["status"] == capi.EDS_OK and o["n"] > 0 for o in outs), outs
            return [t.tolist() for t in trees[0]], trees[1], outs
        return call

    def cloud(count):
        def call(h):
            pts, n = mp.slot_cloud(h, w["T_w_kf"][:count])
            return n, [pts[b, :n[b]] for b in range(count)]
        return call

    return [
        ("build_event_frames", levels(1, 1000), levels(3, 6000)),
        ("build_event_frames_aos", levels_aos(1, 1000), levels_aos(3, 6000)),
        ("build_event_frame_batch", batch(1), batch(3)),
        ("set_undistort_map_sized", lut(H, W), lut(2 * H, 2 * W)),
        ("set_event_frames", upload(1), upload(3)),
        ("update_points_batch", lambda h: h.update_points_batch(0, 1), lambda h: h.update_points_batch(0, 3)),
        ("depth_init + depth_update", depth(1), depth(3)),
        ("klt_track_points", lambda h: h.klt_track_points(0, 1, 3), lambda h: (h.klt_track_points(0, 3, 3), [h.klt_get(s) for s in range(B)])),
        ("epi_track_points", lambda h: h.epi_track_points(0, 1, 3), lambda h: (h.epi_track_points(0, 3, 3), [h.epi_get(s) for s in range(B)])),
        ("refine_points", lambda h: h.refine_points(0, 1, patch_radius=5), lambda h: h.refine_points(0, 3, patch_radius=5)),
        ("project_depth_map", lambda h: h.project_depth_map(0, 1, T7[:1]), lambda h: h.project_depth_map(0, 3, T7)),
        ("build_tree + build_keyframes", keyframes(1, [40]), keyframes(3, [150, 170, 190])),
        ("build_keyframe", lambda h: h.build_keyframe(0, imgs[0], K[0], depth_xy=maps[50][0], depth_idp=maps[50][1], **sel),
         lambda h: h.build_keyframe(0, imgs[0], K[0], depth_xy=maps[500][0], depth_idp=maps[500][1], **sel)),
        ("eds_map_slot_cloud", cloud(1), cloud(3)),
    ]


def test_a_regrown_buffer_serves_as_one_allocated_at_once(gpu, capi, world):
    cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=6)
    grown, fresh = capi.Handle(cfg, B, 256, H, W), capi.Handle(cfg, B, 256, H, W)
    bad = []
    for name, small, large in _steps(world):
        _prepare(grown, world)
        small(grown)
        _prepare(grown, world)
        _prepare(fresh, world)
        bad += [name + d for d in _differ(large(grown), large(fresh))]
    for h in (grown, fresh):
        _prepare(h, world)
        h.optimize_batch(0, 0, B)
    bad += ["optimize_batch" + d for d in _differ((grown.results(0, B), grown.get_states(0, B)), (fresh.results(0, B), fresh.get_states(0, B)))]
    print("\n".join(bad))
    assert not bad, bad
    assert all(i["num_iterations"] > 0 for i in (grown.info(s) for s in range(B)))
    grown.close()
    fresh.close()
