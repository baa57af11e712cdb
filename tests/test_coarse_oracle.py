"""tests/coarse_cases.py discriminates on the numpy oracle alone (tests/np_coarse_oracle.py): every branch of the tracker occurs, the
result changes when the compaction is not row-major, when 1 / n uses the unpadded count, when a collision is summed in another order
and when fx is used for fy; and no accept decision of the loop-parity cases hinges on the last bits of a sum."""
import functools

import numpy as np

import coarse_cases as cc
import np_coarse_oracle as no


@functools.lru_cache(maxsize=None)
def run(name, **variant):
    c = cc.cases()[name]
    o = no.open_case(c, **variant)
    return o, [o.track(T, a, c.coarsest, c.min_res) for T, a in zip(c.T_init, c.aff_init)]


def test_list_shapes_are_the_awkward_ones():
    n0 = {name: len(run(name)[0].pc[0]) for name in ("a64_l3", "b96_l4", "mode_0", "mode_1", "mode_2", "mode_3")}
    assert all(n % 4 and n % 32 and n % 512 for n in n0.values()), n0
    assert n0["b96_l4"] > 512 > n0["mode_0"]
    o = run("empty_top")[0]
    assert len(o.pc[0]) > 0 and len(o.pc[2]) == 0
    a = run("a64_l3")[0]
    assert a.dropped >= 3
    cp = cc.cases()["a64_l3"].cp
    pix = (cp[:, 0] + np.float32(0.5)).astype(int) + 64 * (cp[:, 1] + np.float32(0.5)).astype(int)
    assert (np.unique(pix, return_counts=True)[1] > 1).sum() >= 20                 # several contributions on one pixel
    K = a.K
    assert K[0]["fx"] != K[0]["fy"] and abs(K[0]["cx"] - 31.5) > 1


def test_every_branch_occurs():
    seen = set()
    for name in cc.LOOP_CASES:
        for r in run(name)[1]:
            seen |= r["branches"]
            seen.add("ok" if r["ok"] else "not_ok")
    want = {"cutoff_doubled", "level_repeated", "no_terms", "step_zeroed", "small_inc", "abort", "ok", "not_ok"}
    assert want <= seen, want - seen
    decisions = np.concatenate([r["decisions"] for name in cc.LOOP_CASES for r in run(name)[1]])
    assert (decisions & 1).any() and not (decisions & 1).all()                     # accepts and rejects
    rows = run("a64_l3")[0].calc_res(0, cc.cases()["a64_l3"].T_init[0], (0.0, 0.0), 20.0)["rows"]
    assert rows["warped"].any() and (~rows["in_e"]).any() and (rows["weight"][rows["warped"]] == 1).all()
    jump = run("jump")[0].calc_res(0, cc.IDENT, (0.0, 0.0), 20.0)["rows"]
    assert (jump["in_e"] & ~jump["warped"]).mean() > 0.6                           # saturated terms
    wide = run("jump")[0].calc_res(0, cc.IDENT, (0.0, 0.0), 160.0)["rows"]
    assert (wide["weight"][wide["warped"]] < 1).any()                              # the Huber branch


def test_the_four_affine_modes_differ():
    ends = [run(f"mode_{i}")[1][0] for i in range(4)]
    assert ends[0]["aff"][0] == 0 and ends[0]["aff"][1] == 0 and ends[1]["aff"][1] == 0 and ends[2]["aff"][0] == 0
    assert ends[1]["aff"][0] != 0 and ends[2]["aff"][1] != 0 and ends[3]["aff"][0] != 0 and ends[3]["aff"][1] != 0


def _differs(name, **variant):
    a, b = run(name)[1][0], run(name, **variant)[1][0]
    return not np.array_equal(a["T"], b["T"])


def test_the_variants_the_cases_must_tell_apart():
    # calcRes picks every 32nd entry for the flow indicators: the order of the list is observable there (and, sums being exact here, only there)
    assert not np.array_equal(run("a64_l3")[1][1]["flow"], run("a64_l3", list_order="col")[1][1]["flow"])
    o, v = run("a64_l3")[0], run("a64_l3", list_order="col")[0]
    c = cc.cases()["a64_l3"]
    assert not np.array_equal(o.calc_res(0, c.T_init[1], (0, 0), 20.0)["rs"][[2, 4]], v.calc_res(0, c.T_init[1], (0, 0), 20.0)["rs"][[2, 4]])
    assert _differs("a64_l3", padded=False)
    assert not all(no.same_bits(x, y) for x, y in zip(o.idepth, run("a64_l3", collision_order="reversed")[0].idepth))
    assert _differs("a64_l3", fy_is_fx=True)


def test_no_accept_decision_hinges_on_the_last_bits():
    """Condition of the loop parity: the smallest relative margin |new - old| / old over every accept test is at least 1e-6"""
    margins = {name: min((min(r["margins"]) for r in run(name)[1] if r["margins"]), default=np.inf) for name in cc.LOOP_CASES}
    print(margins)
    assert min(margins.values()) >= 1e-6, margins
