"""Staged consumption in the first-solve tile kernels (csrc/eds_fused.hip, EDS_TILE_STAGES): every lane issues all 32 row
loads of its four points without a branch — a lane that needs nothing of a piece reads a fixed hot line instead — so the compiler counts
vmcnt exactly, and a point's merge, splines and row start behind a wait on that point's own rows while the later points' rows are still in
flight.  The same floats are merged and the arithmetic order is unchanged, so every result must be BIT-IDENTICAL to the build with
predicated loads and one wait for all rows (csrc/libeds_hip_tilestages1.so, -DEDS_TILE_STAGES=1), and agree with the oracle as before.

What can go wrong is a dummy load taken for a real one (or the reverse), a wait that lets a later point's row through, a lane of a ragged
wavefront — not size.  So: the three instantiations that take this path, <0,4,512,1,1,1>, <0,2,512,1,1,1> and <0,2,1024,1,1,1>
(EDS_FORCE_FUSED6), on 64x48 and 48x64 frames with N = 4 (a lone quad), 257 (a ragged last wavefront) and the full fill of 2 000
(1 000 where a lane holds two points), on the scaled frames of tests/test_tile_refetch_gpu.py (patches shift by every amount, are
clamped at edges and leave the frame), each solved twice: from the case's start and warm-started from the first result.  Seeds of the
frames scaled by 0.3 were picked with the oracle on the CPU so that the solves contain, for a whole wavefront of 64 points, passes in
which no point, some points and all points moved their clamped origin — i.e. load instructions that no lane needs, that some lanes
need and that all lanes need; the test checks this on the poses the kernel itself evaluated."""
import dataclasses
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-eds_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
R = importlib.import_module("test_tile_refetch_gpu")          # its cases, its walk along the kernel's trace, its tolerances
ITERS = R.ITERS

# instantiation -> (EDS_FORCE_FUSED6, what last_launch() names, the full fill used here)
INSTANCES = {
    "p4_t512": ("0,4,512,1,1,1", "eds_fused6_kernel<0, 4, 512, 1, 1", 2000),
    "p2_t512": ("0,2,512,1,1,1", "eds_fused6_kernel<0, 2, 512, 1, 1", 1000),
    "p2_t1024": ("0,2,1024,1,1,1", "eds_fused6_kernel<0, 2, 1024, 1, 1", 1000),
}
SHAPES = {"w64": dict(H=48, W=64), "h64": dict(H=64, W=48)}
# (seed, frame scale, N) per slot.  N = 2 000 at scale 0.05, 257 and 4: the slots of test_tile_refetch_gpu.HANDLES; the full fills at
# scale 0.3: oracle runs of seeds 9300-9359 in which at least twelve (wavefront, pass) pairs of the warm-started solve move no origin
SLOTS = {
    ("w64", 2000): [(9254, 0.05, 2000), (9324, 0.3, 2000), (9219, 0.05, 257), (9229, 0.3, 4)],
    ("h64", 2000): [(9228, 0.05, 2000), (9333, 0.3, 2000), (9204, 0.12, 257), (9219, 0.12, 4)],
    ("w64", 1000): [(9340, 0.3, 1000), (9219, 0.05, 257), (9229, 0.3, 4)],
    ("h64", 1000): [(9300, 0.3, 1000), (9204, 0.12, 257), (9219, 0.12, 4)],
}
RUNS = [(inst, shape) for inst in INSTANCES for shape in SHAPES]
CASES = [(inst, shape, b) for inst, shape in RUNS for b in range(len(SLOTS[(shape, INSTANCES[inst][2])]))]

CHILD = r'''
import importlib, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
capi = importlib.import_module("slam-eds_amd.capi"); synth = importlib.import_module("slam-eds_amd.synth")
T = importlib.import_module("test_tile_stages_gpu")
out, kernels = {}, []
def solve(h, P, Q, V, tag):
    B = len(P)
    h.set_states(0, P, Q, V)
    h.optimize_batch(0, 0, B)
    kernels.append(h.last_launch()["kernel"])
    out[tag + "_table"] = h.results(0, B).copy()
    for b in range(B):
        tr = h.trace(b)
        out[f"{tag}_{b}_inc"] = np.asarray(tr["increments"]); out[f"{tag}_{b}_costs"] = np.asarray(tr["costs"]); out[f"{tag}_{b}_acc"] = np.asarray(tr["accepted"])
        out[f"{tag}_{b}_res"] = h.residuals(b).copy()
    return out[tag + "_table"]
for inst, shape in T.RUNS:
    force, _, fill = T.INSTANCES[inst]
    H, W = T.SHAPES[shape]["H"], T.SHAPES[shape]["W"]
    als = [T.R.make_case(synth, s, sc, N, H, W) for s, sc, N in T.SLOTS[(shape, fill)]]
    cfg = capi.default_config(sampling=capi.SAMPLE_BICUBIC, solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=T.ITERS)
    h = capi.Handle(cfg, len(als), fill, H, W)
    h.set_knob("EDS_FORCE_FUSED6", force)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    V = np.stack([a.v0 for a in als])
    t1 = solve(h, np.stack([a.p0 for a in als]), np.stack([a.q0 for a in als]), V, f"{inst}_{shape}_first")
    solve(h, t1[:, 0:3].copy(), t1[:, 3:7].copy(), V, f"{inst}_{shape}_warm")          # warm start: small steps, most rows stay cached
    h.close()
np.savez(sys.argv[2], **out)
print("KERNELS " + " | ".join(kernels))
'''


def _run(lib, path):
    env = dict(os.environ)
    env.pop("EDS_FORCE_FUSED6", None)
    env["EDS_FUSED_LAYOUT"] = "tiles"
    if lib:
        env["EDS_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return [l for l in r.stdout.splitlines() if l.startswith("KERNELS ")][0][8:].split(" | ")


@pytest.fixture(scope="module")
def runs(gpu, capi, tmp_path_factory):
    """The same solves through the product and through the EDS_TILE_STAGES=1 build, one process each (a process holds one library)."""
    ab = os.path.join(CSRC, "libeds_hip_tilestages1.so")
    assert os.path.exists(ab), "csrc/libeds_hip_tilestages1.so is built by __graft_entry__.build() (make libeds_hip_tilestages1.so)"
    d = tmp_path_factory.mktemp("tile_stages")
    ka = _run(None, str(d / "a.npz"))
    kb = _run(ab, str(d / "b.npz"))
    return dict(ka=ka, kb=kb, a=dict(np.load(str(d / "a.npz"))), b=dict(np.load(str(d / "b.npz"))))


@pytest.fixture(scope="module")
def cases(synth):
    return {(shape, fill): [R.make_case(synth, s, sc, N, SHAPES[shape]["H"], SHAPES[shape]["W"]) for s, sc, N in slots] for (shape, fill), slots in SLOTS.items()}


@pytest.fixture(scope="module")
def oracle_runs(po, cases):
    """pose6_lm from every case's own start: computed once, shared by the instantiations."""
    return {(key, b): po.Oracle(al).pose6_lm(al.p0, al.q0, al.v0, iters=ITERS, lambda0=0.01) for key, als in cases.items() for b, al in enumerate(als)}


def _warm(al, table_row):
    return dataclasses.replace(al, p0=table_row[0:3].copy(), q0=table_row[3:7].copy())


def test_forced_instantiations_ran(runs):
    """Both solves of every handle, in both builds, through the forced kernel (last_launch())."""
    assert runs["ka"] == runs["kb"] and len(runs["ka"]) == 2 * len(RUNS)
    for k, (inst, shape) in zip(runs["ka"][0::2] + runs["ka"][1::2], RUNS + RUNS):
        assert k.startswith(INSTANCES[inst][1] + ">") or k.startswith(INSTANCES[inst][1] + ","), (inst, shape, k)


def test_bit_identical_to_the_build_with_one_wait(runs):
    """Poses, iteration counts, traces (increments, costs, accepted) and residuals of every solve, first and warm-started."""
    a, b = runs["a"], runs["b"]
    assert sorted(a) == sorted(b) and len(a) == 2 * sum(1 + 4 * len(SLOTS[(shape, INSTANCES[inst][2])]) for inst, shape in RUNS)
    for k in sorted(a):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    for k in a:
        if k.endswith("_table"):
            assert (a[k][:, 15] == 1.0).all(), k
            assert (a[k][:, 14] == ITERS).all() or not k.endswith("_first_table"), k


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_cases_hold_loads_that_no_some_and_all_lanes_need(runs, cases, po, npo, inst):
    """Per instantiation, on the poses the kernel itself evaluated (its trace): (wavefront, pass) pairs — 64 real points with consecutive
    indices, which one wavefront handles in one of its point slots — in which no point, some points and all points moved their clamped
    origin against the pass before.  (The first pass of a solve, which fetches everything, is not even counted.)"""
    count = dict(none=0, some=0, all=0)
    fill = INSTANCES[inst][2]
    for shape in SHAPES:
        for b, al in enumerate(cases[(shape, fill)]):
            for tag in ("first", "warm"):
                pre = f"{inst}_{shape}_{tag}"
                start = al if tag == "first" else _warm(al, runs["a"][f"{inst}_{shape}_first_table"][b])
                walk = R._patch_walk(po, npo, start, runs["a"][f"{pre}_{b}_inc"], runs["a"][f"{pre}_{b}_acc"])
                for (ra, ca, _, _), (rb, cb, _, _) in zip(walk[:-1], walk[1:]):
                    moved = (ra != rb) | (ca != cb)
                    for s in range(0, al.N - 63, 64):
                        m = int(moved[s:s + 64].sum())
                        count["none" if m == 0 else "all" if m == 64 else "some"] += 1
    print(inst, count)
    assert count["none"] >= 4 and count["some"] >= 4 and count["all"] >= 4, count


@pytest.mark.parametrize("inst,shape,slot", CASES, ids=lambda v: str(v))
def test_against_the_oracle(runs, cases, oracle_runs, po, inst, shape, slot):
    """First solve, as tests/test_tile_refetch_gpu.py checks it and at its tolerances: accept pattern and iteration count of the fp64
    oracle's pose6_lm equal; costs, increments, pose and the residuals at the returned pose (increments and pose not for the four-point
    problems: ill-conditioned, compared between the builds only).  Warm-started solve: it starts at a minimum, where accepting a candidate
    turns on cost differences below fp32 resolution, so the oracle is not asked to take the same decisions — it evaluates every pose the
    kernel evaluated (its trace) and the returned one: candidate costs and residuals at the same tolerances."""
    fill = INSTANCES[inst][2]
    al, ref, a = cases[(shape, fill)][slot], oracle_runs[((shape, fill), slot)], runs["a"]
    pre = f"{inst}_{shape}_first"
    tab = a[pre + "_table"][slot]
    inc, costs, acc, res = a[f"{pre}_{slot}_inc"], a[f"{pre}_{slot}_costs"], a[f"{pre}_{slot}_acc"], a[f"{pre}_{slot}_res"]
    o = po.Oracle(al)
    d_pose = po.se3_distance(tab[0:3], tab[3:7], ref["p"], ref["q"])
    er = o.pose6_eval(tab[0:3], tab[3:7], al.v0)["r"]
    d_res = np.abs(res - er).max() / np.abs(er).max()
    d_cost = np.abs(costs / (0.5 * ref["costs"]) - 1.0).max() if len(costs) == len(ref["costs"]) else np.inf
    steps = [po.se3_distance(*po.se3_exp(inc[k]), *po.se3_exp(ref["increments"][k])) / max(np.linalg.norm(ref["increments"][k]), 1e-3) for k in range(min(len(inc), len(ref["increments"])))]
    print(f"{inst} {shape}[{slot}] N={al.N}: accepted {''.join(map(str, acc))} / {''.join(map(str, ref['accepted']))}  pose {d_pose:.2e}  residuals {d_res:.2e}  costs {d_cost:.2e}  steps {max(steps):.2e}")
    pre = f"{inst}_{shape}_warm"
    tab2 = a[pre + "_table"][slot]
    inc2, costs2, acc2, res2 = a[f"{pre}_{slot}_inc"], a[f"{pre}_{slot}_costs"], a[f"{pre}_{slot}_acc"], a[f"{pre}_{slot}_res"]
    poses = R._evaluated_poses(po, _warm(al, tab), inc2, acc2)
    oc = np.array([o.pose6_eval(p, q, al.v0)["cost"] for p, q in poses[1:]])
    d_cost2 = np.abs(costs2 / (0.5 * oc) - 1.0).max() if len(costs2) == len(oc) >= 1 else np.inf
    er2 = o.pose6_eval(tab2[0:3], tab2[3:7], al.v0)["r"]
    d_res2 = np.abs(res2 - er2).max() / np.abs(er2).max()
    print(f"{inst} {shape}[{slot}] warm: accepted {''.join(map(str, acc2))}  residuals {d_res2:.2e}  candidate costs {d_cost2:.2e}")
    assert np.array_equal(acc, ref["accepted"]) and tab[14] == ref["iterations"] and tab[15] == 1.0
    assert res.shape == (al.N,) and np.isfinite(res).all()
    assert d_cost <= R.TOL_COST_CLAMPED
    assert d_res <= R.TOL_R_CLAMPED
    if al.N >= 257:
        assert max(steps) <= R.TOL_STEP
        assert d_pose <= R.TOL_POSE_CLAMPED
    assert tab2[15] == 1.0 and res2.shape == (al.N,) and np.isfinite(res2).all()
    assert d_cost2 <= R.TOL_COST_CLAMPED
    assert d_res2 <= R.TOL_R_CLAMPED
