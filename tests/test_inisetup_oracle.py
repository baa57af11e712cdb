"""csrc/eds_inisetup.hpp under g++ (tests/inisetup_harness.py) against the numpy restatement of the reference's gridMaxSelection and
makePixelStatus (tests/np_inisetup_oracle.py), EXACTLY, on every case of tests/inisetup_cases.py: maps, numGoodPoints, passes and the
sparsityFactor left behind.  The first test holds the cases themselves to the branches they are there for, on the oracle alone.  No GPU."""
import re

import numpy as np
import pytest

import inisetup_cases as sc
import inisetup_harness as sh
import np_inisetup_oracle as nso


def test_the_cases_cover_the_branches_they_are_there_for():
    a, c, d, e = sc.expected("a"), sc.expected("c"), sc.expected("d"), sc.expected("e")
    assert max(x.passes for x in a) >= 2                                                        # a recursion
    assert any(x.trace[-1][1] == 0.5 for x in a)                                                # a level ends with THFac == 0.5
    assert any(x.trace[-1][0] == 1 for x in a)
    ties = []
    for x in sc.expected("b"):
        for sparsity, th, _ in x.trace:
            if sparsity > 1:
                nso.grid_max_selection(sc.grads("b")[x.lvl], sparsity, th, ties)
    assert len(ties) >= 10, len(ties)                                                           # equal scores inside one cell
    before = [5] + [x.sparsity for x in c[:-1]]
    assert sum(1 for x, b in zip(c, before) if x.sparsity != b) >= 2                            # the carried sparsity changes
    assert any(x.trace[-1][1] == 0.5 for x in c) and len(c) == 4
    assert [x.trace[0][0] for x in d] == [1, 2, 11, 13, 39] and all(x.passes == 1 for x in d)
    assert d[-1].n_good == 0 and not d[-1].map.any() and all(x.n_good > 0 for x in d[:-1])
    assert all(x.n_good == 0 and not x.map.any() for x in e) and e[-1].sparsity == 1
    for name in sc.cases():
        for x in sc.expected(name):
            assert x.n_good == int(x.map.sum()) and 1 <= x.passes <= 6


@pytest.mark.parametrize("name", list(sc.cases()))
def test_host_restatement_equals_the_reference_loop_order(name):
    c, sparsity = sc.cases()[name], 5
    for (lvl, dens, recs, th, set_first), want in zip(c.calls, sc.expected(name)):
        if set_first is not None:
            sparsity = set_first
        status, n_good, passes, sparsity = sh.make_pixel_status(sc.grads(name)[lvl], dens, recs, th, sparsity)
        print(f"{name} level {lvl}: n_good {n_good} passes {passes} sparsity {sparsity}; oracle {want.n_good} {want.passes} {want.sparsity}")
        assert (n_good, passes, sparsity) == (want.n_good, want.passes, want.sparsity)
        assert status.tobytes() == want.map.tobytes()
        for pot, thf, n in want.trace:                                                          # every pass on its own as well
            m, k = sh.grid_max_selection(sc.grads(name)[lvl], pot, thf)
            assert k == n and k == int(m.sum())


def test_single_passes_at_every_cell_size_and_at_the_borders():
    """every pot from 1 to past the level's size on a small level with tied and hostile gradients: the cells' count, the map, numGood"""
    rng = np.random.default_rng(3)
    h, w = 17, 23
    g = np.zeros((h, w, 3), np.float32)
    g[..., 1:] = np.round(rng.normal(0, 12, (h, w, 2))).astype(np.float32)                      # integers: many ties
    g[5, 7, 1], g[6, 2, 2], g[9, 9, 1:] = np.nan, np.inf, (np.inf, np.inf)
    for pot in list(range(1, 25)) + [1000, 1 << 30]:
        want, n = nso.grid_max_selection(g, pot, 1.0)
        got, k = sh.grid_max_selection(g, pot, 1.0)
        assert k == n and got.tobytes() == want.tobytes(), pot
        assert sh.cells(w, pot) == len(range(1, w - pot, pot)) and sh.cells(h, pot) == len(range(1, h - pot, pot))
        if pot >= h - 1:
            assert n == 0


def test_the_controller_at_its_edges():
    g = sc.grads("a")[1]
    for desired, start in ((384.0, -4), (384.0, 0), (1.0, 1), (1e-3, 3), (1e6, 40), (384.0, 1 << 30)):
        for recs in (0, 1, 5):
            want = nso.make_pixel_status(g, desired, recs, 1.0, start)
            got = sh.make_pixel_status(g, desired, recs, 1.0, start)
            assert got[1:] == want[1:] and got[0].tobytes() == want[0].tobytes(), (desired, start, recs)


def test_standalone_program_builds_and_survives_the_hostile_inputs():
    out = sh.run_standalone()
    m = re.search(r"inisetup standalone: (\d+) calls, (\d+) points", out)
    # 4 shapes x (13 + 16) calls of the pixel status, then makeNN over every pair of 10 clouds (level, level above)
    assert m and int(m.group(1)) == 4 * 29 + 10 * 10 and int(m.group(2)) > 100000, out
