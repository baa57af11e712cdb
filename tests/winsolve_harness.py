"""ctypes side of tests/host_logic/winsolve_harness.cpp: csrc/eds_winsolve.hpp (namespace edswsv, what the device kernels run) compiled
with g++ into a temporary directory where the tests run — ``HostWindow`` / ``HostSolver`` have the methods of ``slam-eds_amd.window.Window``
/ ``slam-eds_amd.winsolve.WindowSolver`` — the sequence of calls both sides run over a case, and the stand-alone program of the same
source with the cases dumped for it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import harness_build as hb
import window_harness as wh

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "winsolve_harness.cpp")
OUT_FIELDS = (("adHTdeltaF", "f4", lambda m, n, F, N: (F * F, 8)), ("is_linearized", "i4", lambda m, n, F, N: (m,)),
              ("res_toZeroF", "f4", lambda m, n, F, N: (m, 8)), ("resApprox", "f4", lambda m, n, F, N: (m, 8)), ("lf", "f4", lambda m, n, F, N: (n, 6)),
              ("HFinal", "f8", lambda m, n, F, N: (N, N)), ("bFinal", "f8", lambda m, n, F, N: (N,)), ("xAd", "f4", lambda m, n, F, N: (F * F, 8)),
              ("frame_step", "f8", lambda m, n, F, N: (N,)), ("step", "f4", lambda m, n, F, N: (n,)), ("idepth_scaled", "f4", lambda m, n, F, N: (n,)),
              ("priorF", "f4", lambda m, n, F, N: (n,)))
SYSTEM_FIELDS = ("HFinal", "bFinal", "xAd", "frame_step")
OK, INVALID, NOT_USABLE, STATE = 0, -1, -3, -4
_WIN_FUNCS = ("win_create", "win_destroy", "win_set_params", "win_set_calib", "win_set_frames", "win_get_frame", "win_set_points", "win_set_idepths",
              "win_set_residuals", "win_linearize", "win_apply", "win_point_hessians", "win_get_residuals", "win_accumulate", "win_get_points",
              "win_stitch_entries", "win_linearize_points", "win_linearize_fold", "win_apply_points", "win_point_hessians_points")


class Stats(C.Structure):
    _fields_ = [("res_in_a", C.c_int32), ("res_in_l", C.c_int32), ("orthogonalized_x", C.c_int32), ("orthogonalized_system", C.c_int32),
                ("lambda_", C.c_double)]


class HostError(RuntimeError):
    def __init__(self, code):
        super().__init__(f"edswsv harness refused: {code}")
        self.code = code


_lib = None


def load_harness():
    """the library of winsolve_harness.cpp: window_harness.cpp's functions (bound as window_harness binds them) and the wsv_* ones"""
    global _lib
    if _lib is None:
        L = hb.load_library("winsolve", SRC)
        base = wh.load_harness()
        for name in _WIN_FUNCS:
            f, g = getattr(L, name), getattr(base, name)
            f.argtypes, f.restype = g.argtypes, g.restype
        vp, d, fl, i = C.c_void_p, C.c_double, C.c_float, C.c_int
        L.wsv_create.restype = vp
        L.wsv_create.argtypes = [vp]
        L.wsv_destroy.argtypes = [vp]
        L.wsv_invalidate.argtypes = [vp]
        L.wsv_set_state.argtypes = [vp, i] + [vp] * 9
        L.wsv_fix_linearization.argtypes = [vp, vp]
        L.wsv_solve.argtypes = [vp, i, d, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
        L.wsv_backup_idepths.argtypes = [vp]
        L.wsv_step_idepths.argtypes = [vp, fl]
        L.wsv_l_energy.argtypes = [vp, vp]
        L.wsv_l_energy_points.argtypes = [vp, vp]
        L.wsv_m_energy.argtypes = [vp, vp, vp, vp]
        L.wsv_marginalize_points.argtypes = [vp, vp, fl, d, vp, vp, vp]
        L.wsv_get.argtypes = [vp, vp]
        L.wsv_get_acc.argtypes = [vp, vp, vp, vp, vp]
        L.wsv_ldlt.argtypes = [i, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


class HostWindow(wh.HostWindow):
    """window_harness.HostWindow over this library, so that a HostSolver can stand on it"""

    def __init__(self, H, W, max_frames=8, **params):
        self.L = load_harness()
        self.H, self.W, self.max_frames = H, W, max_frames
        self._h = self.L.win_create(H, W, max_frames)
        assert self._h, "shape refused"
        self.prm = dict(wh.DEFAULTS)
        self.n = self.m = 0
        self.solver = None
        if params:
            self.set_params(**params)

    def set_points(self, *a, **k):
        super().set_points(*a, **k)
        if self.solver:
            self.solver.invalidate()

    def set_residuals(self, *a, **k):
        super().set_residuals(*a, **k)
        if self.solver:
            self.solver.invalidate()


_vp = hb.p


def _f64(a, shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def _rc(code):
    if code != OK:
        raise HostError(code)


class HostSolver:
    """edswsv:: under g++ behind the interface of slam-eds_amd.winsolve.WindowSolver"""

    def __init__(self, win):
        self.L = load_harness()
        self.win, self.F = win, 0
        self._s = self.L.wsv_create(win._h)
        win.solver = self

    def close(self):
        if self._s:
            self.L.wsv_destroy(self._s)
            self._s = None

    def invalidate(self):
        self.L.wsv_invalidate(self._s)

    @property
    def N(self):
        return 4 + 8 * self.F

    def set_state(self, F, adHost, adTarget, delta, prior, delta_prior, cPrior, cDelta, priorF=None, deltaF=None):
        pf = None if priorF is None else wh._f32(priorF, (self.win.n,))
        df = None if deltaF is None else wh._f32(deltaF, (self.win.n,))
        _rc(self.L.wsv_set_state(self._s, F, _vp(_f64(adHost, (F * F, 8, 8))), _vp(_f64(adTarget, (F * F, 8, 8))), _vp(_f64(delta, (F, 8))),
                                 _vp(_f64(prior, (F, 8))), _vp(_f64(delta_prior, (F, 8))), _vp(_f64(cPrior, (4,))), _vp(_f64(cDelta, (4,))), _vp(pf), _vp(df)))
        self.F = F

    def fix_linearization(self, select):
        _rc(self.L.wsv_fix_linearization(self._s, _vp(np.ascontiguousarray(select, dtype=np.int32).reshape(self.win.m))))

    def solve(self, iteration, lam, HM, bM, mode, have_first_frame=True, projector=None):
        N = self.N
        P = None if projector is None else _f64(projector, (N, N))
        out = dict(x=np.zeros(N), lastHS=np.zeros((N, N)), lastbS=np.zeros(N))
        st = Stats()
        _rc(self.L.wsv_solve(self._s, int(iteration), float(lam), int(mode), 1 if have_first_frame else 0, _vp(_f64(HM, (N, N))), _vp(_f64(bM, (N,))), _vp(P),
                             _vp(out["x"]), _vp(out["lastHS"]), _vp(out["lastbS"]), C.byref(st)))
        out.update(res_in_a=st.res_in_a, res_in_l=st.res_in_l, lam=st.lambda_, orthogonalized_x=st.orthogonalized_x,
                   orthogonalized_system=st.orthogonalized_system)
        return out

    def backup_idepths(self):
        _rc(self.L.wsv_backup_idepths(self._s))

    def step_idepths(self, fac=1.0):
        _rc(self.L.wsv_step_idepths(self._s, float(fac)))

    def steps(self):
        return self.get(system=False)["step"]

    def l_energy(self):
        e = C.c_double()
        _rc(self.L.wsv_l_energy(self._s, C.cast(C.byref(e), C.c_void_p)))
        return e.value

    def l_energy_points(self):
        out = np.zeros(self.win.n)
        self.L.wsv_l_energy_points(self._s, _vp(out))
        return out

    def m_energy(self, HM, bM):
        N = self.N
        e = C.c_double()
        _rc(self.L.wsv_m_energy(self._s, _vp(_f64(HM, (N, N))), _vp(_f64(bM, (N,))), C.cast(C.byref(e), C.c_void_p)))
        return e.value

    def marginalize_points(self, marg, HM, bM, prior_fac=1.0, weight_fac=1.0):
        N = self.N
        hm, bm = _f64(HM, (N, N)).copy(), _f64(bM, (N,)).copy()
        res = C.c_int32()
        _rc(self.L.wsv_marginalize_points(self._s, _vp(np.ascontiguousarray(marg, dtype=np.int32).reshape(self.win.n)), float(prior_fac), float(weight_fac),
                                          _vp(hm), _vp(bm), C.cast(C.byref(res), C.c_void_p)))
        return hm, bm, res.value

    def get(self, system=True):
        m, n, F, N = self.win.m, self.win.n, self.F, self.N
        out = {k: np.zeros(sh(m, n, F, N), dt) for k, dt, sh in OUT_FIELDS}
        ptrs = [out[k].ctypes.data if (system or k not in SYSTEM_FIELDS) else 0 for k, _, _ in OUT_FIELDS]
        _rc(self.L.wsv_get(self._s, struct.pack(f"<{len(ptrs)}Q", *ptrs)))
        return {k: v for k, v in out.items() if system or k not in SYSTEM_FIELDS}

    def raw(self):
        """the last pass's accumulators (mode 0 and the Schur complement after a solve, mode 2 after a marginalisation), mode 1's top accumulators, its stitch (H_L, b_L before the priors) and mode 0's / the Schur complement's stitch of the last solve"""
        F, N = self.F, self.N
        accL, stL, st = np.zeros(F * F * 92), np.zeros(N * (N + 1)), np.zeros(2 * N * (N + 1))
        acc = np.zeros(self.L.win_acc_size(F))
        self.L.wsv_get_acc(self._s, _vp(accL), _vp(stL), _vp(st), _vp(acc))
        half = N * (N + 1)
        return dict(acc=acc, accL=accL, H_L=stL[:N * N].reshape(N, N), b_L=stL[N * N:], H_A=st[:N * N].reshape(N, N), b_A=st[N * N:half],
                    H_sc=st[half:half + N * N].reshape(N, N), b_sc=st[half + N * N:])


def ldlt(H, b):
    """the stated LDLT alone: (x, L, d, perm)"""
    N = len(b)
    H, b = _f64(H, (N, N)), _f64(b, (N,))
    x, L, dp = np.zeros(N), np.zeros((N, N)), np.zeros((2, N))
    rc = load_harness().wsv_ldlt(N, _vp(H), _vp(b), _vp(x), _vp(L), _vp(dp))
    assert rc in (OK, NOT_USABLE)
    return x, L, dp[0], dp[1].astype(int)


def open_case(s, win_cls=HostWindow, solver_cls=HostSolver, **kw):
    w = wh.open_case(s.win, win_cls, **kw)
    return w, solver_cls(w)


def lin_apply(w, s):
    c = s.win
    w.linearize(c.F, c.precalc, c.th)
    w.apply(True)


def run_sequence(w, sv, s, probe=None):
    """the calls of one optimisation over case s, and everything a caller can read after each: linearize -> apply -> set_state ->
    fix_linearization; per round backup -> solve -> both energies -> step -> linearize -> apply; then the residuals of the flagged
    points are fixed, the points marginalised, and a last solve runs with the updated HM, bM.  probe(tag, w, sv) may look in between."""
    c = s.win
    out = []
    lin_apply(w, s)
    sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, s.priorF, s.deltaF)
    sv.fix_linearization(s.fix)
    out.append(dict(tag="fixed", state=sv.get(system=False)))
    for k, r in enumerate(s.rounds):
        sv.backup_idepths()
        sol = sv.solve(r.iteration, r.lam, s.HM, s.bM, r.mode, r.hff, s.P if r.use_p else None)
        if probe:
            probe(f"round{k}", w, sv)
        rec = dict(tag=f"round{k}", solve=sol, state=sv.get(), points=w.points(), steps=sv.steps(), l_energy=np.float64(sv.l_energy()),
                   m_energy=np.float64(sv.m_energy(s.HM, s.bM)))
        sv.step_idepths(r.fac)
        rec["stepped"] = sv.get(system=False)["idepth_scaled"]
        lin_apply(w, s)
        rec["relinearized"] = w.residuals()
        out.append(rec)
    sv.fix_linearization(s.fix_marg)
    HM, bM, res_m = sv.marginalize_points(s.marg, s.HM, s.bM, prior_fac=PRIOR_FAC, weight_fac=WEIGHT_FAC)
    if probe:
        probe("marg", w, sv)
    sol = sv.solve(0, 0.0, HM, bM, DEFAULT_MODE, True, None)
    out.append(dict(tag="marginalised", HM=HM, bM=bM, res_in_m=np.int32(res_m), solve=sol, state=sv.get(), points=w.points()))
    return out


PRIOR_FAC, WEIGHT_FAC, DEFAULT_MODE = 2.0, 0.25, 128 | 2048


def flatten(tree, prefix=""):
    """every array of a nested result, by path"""
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from flatten(v, f"{prefix}/{k}")
    elif isinstance(tree, (list, tuple)):
        for k, v in enumerate(tree):
            yield from flatten(v, f"{prefix}[{k}]")
    elif isinstance(tree, str):
        return
    else:
        yield prefix, np.asarray(tree)


def same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return bool((na == nb).all() and a[~na].tobytes() == b[~nb].tobytes())
    return a.tobytes() == b.tobytes()


def dump_cases(path, cases):
    """the binary the stand-alone program reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for s in cases:
            c = s.win
            prm = dict(wh.DEFAULTS)
            prm.update(c.prm)
            f.write(struct.pack("<6i", c.H, c.W, c.F, len(c.host), len(c.point), int(c.shift)) + wh.pack_params(prm) + struct.pack("<4f", *c.K))
            for a, dt in ((c.images, "f4"), (c.host, "i4"), (c.uv, "f4"), (c.color, "f4"), (c.weights, "f4"), (c.ids, "f4"), (c.idz, "f4"),
                          (c.point, "i4"), (c.target, "i4"), (c.state, "i4"), (c.energy, "f4"), (c.precalc, "f4"), (c.th, "f4"), (s.priorF, "f4"),
                          (s.deltaF, "f4"), (c.adH, "f8"), (c.adT, "f8"), (s.delta, "f8"), (s.prior, "f8"), (s.delta_prior, "f8"), (s.cPrior, "f8"),
                          (s.cDelta, "f8"), (s.HM, "f8"), (s.bM, "f8"), (s.P, "f8"), (s.fix, "i4"), (s.marg, "i4")):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())


def run_standalone(cases, extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -g -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once over
    `cases` plus its own hostile inputs, returns its output; raises when it fails"""
    exe, data = hb.build_program("winsolve", SRC, "WSV_STANDALONE", extra_flags)
    dump_cases(data, cases)
    return subprocess.check_output([exe, data], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/winsolve_harness.py [g++ flags]: the sanitizer run of DESIGN §18
    import sys
    sys.path.insert(0, HERE)
    import winsolve_cases as wsc
    print(run_standalone(list(wsc.cases().values()), sys.argv[1:]), end="")
