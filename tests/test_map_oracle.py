"""csrc/eds_map.hpp (namespace edsmap — what the map kernels run, compiled here with g++) against the numpy restatement of the reference's
getMap, getImmatureMap, KeyFrame::getMap and IDepthMap::fromPoints (np_map_oracle.py), bit for bit on every case.  No GPU."""
import subprocess

import numpy as np
import pytest

import map_cases as mc
import map_harness as mh
import np_map_oracle as mo


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(mo.bits(a), mo.bits(b))


@pytest.fixture(scope="module")
def cases():
    edge, _ = mc.edge_case()
    return mc.window_cases(mh.chunk()) + [mc.degenerate_case(), mc.plane_case(), edge]


def test_chunk_is_a_whole_number_of_wavefronts():
    assert mh.chunk() % 64 == 0 and mh.chunk() >= 64


def test_window_cloud_equals_the_oracle(cases):
    for c in cases:
        for single in (True, False):
            got, per = mh.window_cloud(c["host"], c["uv"], c["ids"], c["calib"], c["T_w_c"], c["mask"], single)
            ref, per_ref = mo.window_cloud(c["host"], c["uv"], c["ids"], c["calib"], c["T_w_c"], c["mask"], single)
            assert same(got, ref) and np.array_equal(per, per_ref), (c["name"], single)
            assert len(got) == mc.selected(c) * (1 if single else 8)


def test_the_fan_is_the_reference_order():
    """the eight points of one point, by hand: the centre, then (0,+2) (-1,+1) (-2,0) (-1,-1) (0,-2) (+1,-1) (+2,0)"""
    eye = mc.pose(np.eye(3), [0, 0, 0])
    got, _ = mh.window_cloud([0], [[10.0, 20.0]], [0.5], [1, 1, 0, 0], [eye, eye], 1, False)
    assert got.tolist() == [[2 * (10 + du), 2 * (20 + dv), 2.0] for du, dv in ((0, 0), (0, 2), (-1, 1), (-2, 0), (-1, -1), (0, -2), (1, -1), (2, 0))]


def test_depth_maps_equal_the_oracle(cases):
    for c in cases:
        args = (c["host"], c["uv"], c["ids"], c["calib"], c["T_w_c"], c["mask"], c["T_dst_w"], c["K_dst"], c["dst_H"], c["dst_W"])
        got, ref = mh.window_depth_maps(*args), mo.window_depth_maps(*args)
        assert len(got) == len(ref) == len(c["T_dst_w"])
        for b, (g, r) in enumerate(zip(got, ref)):
            assert same(g["xy"], r["xy"]) and same(g["idp"], r["idp"]) and same(g["src"], r["src"]), (c["name"], b)


def test_a_batch_of_maps_equals_its_singles(cases):
    for c in cases:
        args = (c["host"], c["uv"], c["ids"], c["calib"], c["T_w_c"], c["mask"])
        batch = mh.window_depth_maps(*args, c["T_dst_w"], c["K_dst"], c["dst_H"], c["dst_W"])
        for b in range(len(batch)):
            one = mh.window_depth_maps(*args, c["T_dst_w"][b:b + 1], c["K_dst"][b:b + 1], c["dst_H"], c["dst_W"])[0]
            assert all(same(one[k], batch[b][k]) for k in ("xy", "idp", "src")), (c["name"], b)


def test_inlier_edges_land_where_intended():
    c, expect = mc.edge_case()
    m = mh.window_depth_maps(c["host"], c["uv"], c["ids"], c["calib"], c["T_w_c"], c["mask"], c["T_dst_w"], c["K_dst"], c["dst_H"], c["dst_W"])
    for b, e in enumerate(expect):
        for i, kept in e.items():
            assert (i in m[b]["src"]) == kept, (b, i)


def test_immature_cloud_equals_the_oracle():
    for c in mc.immature_cases(mh.chunk()):
        alive = mc.pattern_alive(c["uv"], mc.WIN_H, mc.WIN_W)
        assert 0 < alive.sum() < len(alive) or not len(alive)
        for single in (True, False):
            args = (c["per_host"], c["uv"].astype(np.float32), c["idepth_min"], c["idepth_max"], c["status"], alive, c["T_w_c"], c["calib"], c["mask"], single)
            got, ref = mh.immature_cloud(*args), mo.immature_cloud(*args)
            assert all(same(got[k], ref[k]) for k in ("points", "colors", "status")), (c["name"], single)
            if c["mask"]:
                assert 0 < len(ref["points"]) < sum(c["per_host"]) * (1 if single else 8)
                assert set(ref["status"].tolist()) == set(range(6))


def test_slot_cloud_equals_the_oracle():
    for seed, n in ((41, 0), (42, 1), (43, 257)):
        c = mc.slot_case(seed, n)
        assert same(mh.slot_cloud(c["xn"], c["yn"], c["idp"], c["T_w_kf"]), mo.slot_cloud(c["xn"], c["yn"], c["idp"], c["T_w_kf"]))


def test_standalone_program_runs_the_cases(cases):
    """the same source under its own main, as a sanitizer build runs it: every case through buffers of exactly the needed size"""
    exe, data = mh.standalone(cases)
    out = subprocess.check_output([exe, data], text=True)
    assert out.startswith(f"{len(cases)} cases")
