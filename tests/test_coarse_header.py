"""include/eds_hip_coarse.h, the companion header of the coarse image tracker: plain C like eds_hip.h, every function it declares is
exported by libeds_hip.so and listed in capi.CT_EXPORTS, and its defaults are the reference's settings table; and csrc/eds_coarse.hpp
under g++ (tests/coarse_harness.py): its own sin, cos and exp against libm within the bounds the header states, the sum order's fold,
and the properties of the serial restatement that need no oracle (no GPU needed: nothing here launches anything)."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import coarse_cases as cc
import coarse_harness as ch
import header_checks as hc

capi = hc.capi
coarse = importlib.import_module("slam-eds_amd.coarse")

# reference src/utils/settings.cpp:119-138
REFERENCE_SETTINGS = dict(huber_th=9.0, coarse_cutoff_th=20.0, affine_opt_mode_a=1e12, affine_opt_mode_b=1e8)


def test_coarse_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_coarse.h", hc.declared("eds_hip_coarse.h"), [
        "    eds_ct_params p; eds_ct_result r;",
        "    float x = 0; double d[12] = {0}; int32_t m = 0;",
        "    if (eds_ct_abi_version() != EDS_HIP_COARSE_ABI_VERSION || EDS_HIP_COARSE_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6) return 4;",
        "    eds_ct_params_default(&p);",
        "    if (p.huber_th != 9.0f || p.coarse_cutoff_th != 20.0f || p.affine_opt_mode_a != 1e12f || p.affine_opt_mode_b != 1e8f) return 5;",
        "    if (eds_ct_set_params(0, &p) != EDS_ERR_INVALID || eds_ct_get_params(0, &p) != EDS_ERR_INVALID) return 6;",
        "    if (eds_ct_create(0, 64, 64, 5, 1, 1, 0) != EDS_ERR_INVALID) return 7;",
        "    if (eds_ct_set_calib(0, 1, 1, 0, 0) != EDS_ERR_INVALID || eds_ct_get_k(0, 0, &x) != EDS_ERR_INVALID) return 8;",
        "    if (eds_ct_set_ref(0, &x, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID || eds_ct_set_new(0, &x, 0, 0, 1) != EDS_ERR_INVALID) return 9;",
        "    if (eds_ct_track(0, 1, d, d, 0, d, &r) != EDS_ERR_INVALID || eds_ct_calc_res(0, 0, d, d, 20, 0, 0, 0, 0) != EDS_ERR_INVALID) return 10;",
        "    if (eds_ct_get_level(0, EDS_CT_PC, 0, &x, &m) != EDS_ERR_INVALID) return 11;",
        "    if (sizeof(eds_ct_row) != 64 || sizeof(eds_ct_result) != 744 || EDS_CT_MAX_LEVELS != 5 || EDS_CT_PC != 4) return 12;",
        "    eds_ct_destroy(0);"], tmp_path)


def test_defaults_equal_the_reference_settings():
    p = coarse.default_params()
    want = {k: C.c_float(v).value for k, v in REFERENCE_SETTINGS.items()}
    assert p.as_dict() == want
    assert [k for k, _ in coarse.Params._fields_] == list(REFERENCE_SETTINGS) == list(ch.PARAM_ORDER)
    assert coarse.RESULT == ch.RESULT and coarse.ROW == ch.ROW


def test_coarse_sources_are_build_inputs():
    for f in ("eds_coarse.hip", "eds_hip_coarse.h", "eds_coarse.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp", "eds_dso_image.hip"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_coarse.o")) and hc.contraction_off(hc.resources_line("eds_coarse.hip"))


def _ulps(got, want):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_own_sincos_and_exp_are_within_the_stated_ulps_of_libm():
    """the arguments the loop can produce: the rotation angle of an increment and its half (|x| <= 4), a difference of affine a's
    (|x| <= 3) — which the loop does not bound, so the samples cover everything the functions accept (|x| <= 2^20 and |x| <= 708) and
    the small arguments densely; the bounds are the header's constants (measured: sin 2, cos 2, exp 1)"""
    rng = np.random.default_rng(0)
    L = ch.load_harness()
    sincos_ulp, exp_ulp = C.c_int(), C.c_int()
    L.ct_ulp_bounds(C.byref(sincos_ulp), C.byref(exp_ulp))
    hdr = open(os.path.join(capi.CSRC, "eds_coarse.hpp")).read()
    assert f"SINCOS_MAX_ULP = {sincos_ulp.value};" in hdr and f"EXP_MAX_ULP = {exp_ulp.value};" in hdr
    x = np.concatenate([rng.uniform(-4, 4, 100000), np.linspace(-4, 4, 4001), 10.0 ** rng.uniform(-12, 0, 20000), rng.uniform(-100, 100, 50000),
                        rng.uniform(-2.0 ** 20, 2.0 ** 20, 100000), np.arange(-3000, 3000) * (math.pi / 2), [0.0, math.pi / 4, -math.pi / 4]])
    s, c = ch.sincos(x)
    es = _ulps(s, [math.sin(v) for v in x]).max()
    ec = _ulps(c, [math.cos(v) for v in x]).max()
    y = np.concatenate([rng.uniform(-3, 3, 100000), np.linspace(-3, 3, 3001), rng.uniform(-40, 40, 50000), rng.uniform(-708, 708, 100000), [0.0]])
    ee = _ulps(ch.exp(y), [math.exp(v) for v in y]).max()
    print(f"max ulps: sin {es:.2f} cos {ec:.2f} exp {ee:.2f}")
    assert es <= sincos_ulp.value and ec <= sincos_ulp.value and ee <= exp_ulp.value
    s, c = ch.sincos(np.array([np.nan, np.inf, -np.inf, 1e300]))
    assert np.isnan(s).all() and np.isnan(c).all()
    e = ch.exp(np.array([np.nan, 800.0, -800.0, np.inf, -np.inf]))
    assert np.isnan(e[0]) and e[1] == np.inf and e[2] == 0 and e[3] == np.inf and e[4] == 0


def test_shapes_the_header_refuses():
    L = ch.load_harness()
    assert L.ct_shape_valid(48, 64, 3) and L.ct_shape_valid(64, 96, 4) and L.ct_shape_valid(480, 640, 5) and L.ct_shape_valid(8, 8, 1)
    for H, W, lv in ((48, 64, 4), (50, 64, 3), (48, 66, 3), (48, 64, 0), (48, 64, 6), (4, 64, 1), (16384, 64, 1)):
        assert not L.ct_shape_valid(H, W, lv), (H, W, lv)


def test_serial_restatement_tracks_the_known_motion_and_repeats():
    c = cc.cases()["b96_l4"]
    t = ch.open_case(c)
    r = t.track(c.T_init, c.aff_init, c.coarsest, c.min_res)
    assert r["ok"].all()
    for k in range(len(r)):
        assert np.abs(r["T"][k] - c.T_true).max() < 5e-3, np.abs(r["T"][k] - c.T_true).max()
        assert r["iterations"][k].sum() == r["n_decisions"][k] and r["accepts"][k].sum() == (r["decisions"][k][:r["n_decisions"][k]] & 1).sum()
    assert r.tobytes() == t.track(c.T_init, c.aff_init, c.coarsest, c.min_res).tobytes()
    singles = np.concatenate([t.track(c.T_init[k], c.aff_init[k], c.coarsest, c.min_res) for k in range(len(r))])
    assert singles.tobytes() == r.tobytes()
    t.close()


# ---- edsct:: under g++ against the numpy oracle (tests/np_coarse_oracle.py) ---------------------------------------------------------------
import functools

import np_coarse_oracle as no

# measured on these cases (the solve's and libm's roundings only): 1.8e-15 on a pose entry, 1.5e-13 on the affine pair; asserted with one
# order of magnitude over
POSE_BOUND, AFF_BOUND = 2e-14, 1.5e-12
ROW_FIELDS = ("idepth", "u", "v", "dx", "dy", "residual", "weight", "ref_color")


@functools.lru_cache(maxsize=None)
def _pair(name):
    c = cc.cases()[name]
    return c, ch.open_case(c), no.open_case(c)


def _within(got, want, bound):
    with np.errstate(all="ignore"):
        return bool(((np.abs(got - want) <= bound) | (np.isnan(got) & np.isnan(want)) | (got == want)).all())


@pytest.mark.parametrize("name", list(cc.cases()))
def test_pyramids_depth_maps_and_lists_equal_the_oracle_bit_for_bit(name):
    c, t, o = _pair(name)
    assert t.set_ref(c.ref, c.cp, c.hdif, c.exposure_ref, c.aff_ref)[1] == o.dropped
    assert [int(n) for n in t.pc_n] == [len(p) for p in o.pc]
    for l in range(c.levels):
        k = o.K[l]
        assert no.same_bits(t.K(l), np.array([k["fx"], k["fy"], k["cx"], k["cy"]], np.float32))
        for which, ref in ((ch.REF_IMAGE, o.ref[l]), (ch.NEW_IMAGE, o.new[l]), (ch.IDEPTH, o.idepth[l]), (ch.WEIGHT_SUMS, o.wsum[l]), (ch.PC, o.pc[l])):
            assert no.same_bits(t.level(which, l), np.ascontiguousarray(ref, dtype=np.float32)), (name, l, which)


@pytest.mark.parametrize("name", list(cc.cases()))
def test_rows_equal_the_oracle_and_sums_are_within_the_derived_bound(name):
    """every per-point value bit for bit; E, H and b within n 2^-53 sum|term| of the exact sum of the same fp32 terms"""
    c, t, o = _pair(name)
    for T, a in zip(c.T_init, c.aff_init):
        for l in range(c.levels):
            for cutoff in (20.0, 160.0) if l == 0 else (20.0,):
                g = t.calc_res(l, T, a, cutoff)
                res, H, b, Hb, bb = o.system(l, T, a, np.float32(cutoff))
                rows = res["rows"]
                for f in ch.ROW.names:
                    m = rows["warped"] if f in ROW_FIELDS else rows["flow"] if f.startswith("shift") else np.ones(len(g["rows"]), bool)
                    assert no.same_bits(g["rows"][f][m], np.asarray(rows[f])[m].astype(ch.ROW[f])), (name, l, f)
                assert _within(g["rs"][0], res["rs"][0], res["abs"]["n"] * 2.0 ** -53 * res["abs"]["E"])
                assert np.array_equal(g["rs"][[1, 3, 5]], res["rs"][[1, 3, 5]], equal_nan=True)
                assert _within(g["rs"][2:5], res["rs"][2:5], no.flow_bound(res)), (name, l)
                assert _within(g["H"], H, Hb) and _within(g["b"], b, bb), (name, l)


@pytest.mark.parametrize("name", cc.LOOP_CASES)
def test_the_loop_equals_the_oracle(name):
    """the accept sequence, the iteration counts and the bool are identical; pose and affine pair within the measured bound"""
    c, t, o = _pair(name)
    r = t.track(c.T_init, c.aff_init, c.coarsest, c.min_res)
    for k, (T, a) in enumerate(zip(c.T_init, c.aff_init)):
        q = o.track(T, a, c.coarsest, c.min_res)
        assert list(r["decisions"][k][:r["n_decisions"][k]]) == q["decisions"]
        assert np.array_equal(r["iterations"][k], q["iterations"]) and np.array_equal(r["accepts"][k], q["accepts"])
        assert bool(r["ok"][k]) == q["ok"] and r["level_cutoff_repeat"][k] == q["cutoff_repeat"]
        dT, da = np.abs(r["T"][k] - q["T"]).max(), np.abs(r["aff"][k] - q["aff"]).max()
        print(f"{name}[{k}]: |dT| {dT:.3g} |daff| {da:.3g}")
        assert dT <= POSE_BOUND and da <= AFF_BOUND
        assert np.array_equal(r["last_residuals"][k], q["last_residuals"], equal_nan=True)
        # the same derived bound as for rs: the terms are the oracle's bit for bit as long as the two poses narrow to the same floats,
        # which the exact equality of lastResiduals above already requires
        assert _within(r["last_flow_indicators"][k], q["flow"], q["flow_bound"]), (r["last_flow_indicators"][k], q["flow"], q["flow_bound"])
        R = r["T"][k][:, :3]
        drift = np.abs(R.T @ R - np.eye(3)).max()
        print(f"{name}[{k}]: |R^T R - I| {drift:.3g} after {r['n_decisions'][k]} products")
        # the pose is a matrix updated by Rinc R without re-normalisation: each product adds a few roundings, 8 ulps of 1 allowed per product
        assert drift <= (1 + r["n_decisions"][k]) * 8 * 2.0 ** -53


def test_standalone_program_builds_and_survives_the_hostile_inputs():
    """the program of the sanitizer run, built plainly: all cases plus NaN / inf poses, intrinsics, affine pairs and
    exposures, zero and negative HdiF, contributions at +-2^31, the empty reference"""
    out = ch.run_standalone(list(cc.cases().values()))
    m = re.search(r"coarse standalone: (\d+) cases; (\d+) tracks, (\d+) ok, (\d+) iterations, (\d+) list entries evaluated", out)
    assert m, out
    n_cases, tracks, ok, iters, entries = (int(v) for v in m.groups())
    assert n_cases == len(cc.cases()) and tracks > 1000 and 0 < ok < tracks and iters > tracks and entries > 10 ** 6
