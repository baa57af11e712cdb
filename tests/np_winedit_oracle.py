"""An independent statement of include/eds_hip_winedit.h in numpy: a snapshot of every row a caller can read (tests/winedit_harness.py
``snapshot``) gathered by the indices of the survivors.  Plain index gathers — ``numpy.flatnonzero`` and fancy indexing; it knows
nothing of prefix sums, second buffers or 16-byte pieces.  ``mutate`` names a deliberate error, for the tests that show the comparison
can fail: every mutation changes the result of at least one case."""
import numpy as np

IN = 0
MUTATIONS = ("unstable_order", "points_not_renumbered", "stale_res_first", "residuals_of_removed_points_kept", "select_null_keeps_outliers",
             "solver_rows_left_behind")
FRAME_MUTATIONS = ("targets_not_renumbered", "hosts_not_renumbered", "residuals_towards_the_frame_kept")
ARITH_MUTATIONS = ("permutation_off_by_one_block", "prior_not_added", "unscale_by_SI", "missing_symmetrisation", "sum_descending")

PER_RESIDUAL = (("residuals", None), ("state", ("is_linearized", "res_toZeroF", "resApprox")), ("rows", ("target",)))
PER_POINT = (("points", None), ("state", ("lf", "step", "idepth_scaled", "priorF")),
             ("rows", ("host", "uv", "color", "weights", "idepth_zero_scaled", "deltaF", "idepth_backup")))


def _swap_with_back(keep):
    """the order the reference's removePoint / dropResidual leave: each removed element's hole is filled by the current last one"""
    order = list(range(len(keep)))
    gone = [i for i in range(len(keep)) if not keep[i]]
    for i in gone:
        k = order.index(i)
        order[k] = order[-1]
        order.pop()
    return np.array(order, dtype=np.int64)


def survivors(snap, point_flag=None, select=None, mutate=None, frame=None):
    """(indices of the surviving points, indices of the surviving residuals), both increasing"""
    n, m = int(snap["counts"][0]), int(snap["counts"][1])
    point = snap["rows"]["point"]
    keep_p = np.ones(n, bool) if point_flag is None else np.asarray(point_flag).reshape(n) == 0
    if frame is not None:
        keep_r = snap["rows"]["target"] != frame if mutate != "residuals_towards_the_frame_kept" else np.ones(m, bool)
    elif point_flag is not None:
        keep_r = keep_p[point] if mutate != "residuals_of_removed_points_kept" else np.ones(m, bool)
    elif select is not None:
        keep_r = np.asarray(select).reshape(m) == 0
    else:
        keep_r = snap["residuals"]["state"] == IN
        if mutate == "select_null_keeps_outliers":
            keep_r = snap["residuals"]["state"] != 1
    if mutate == "unstable_order":
        return _swap_with_back(keep_p), _swap_with_back(keep_r)
    return np.flatnonzero(keep_p), np.flatnonzero(keep_r)


def edit(snap, point_flag=None, select=None, mutate=None, frame=None):
    """the snapshot after eds_wed_remove_points(point_flag), eds_wed_remove_residuals(select) or the table half of
    eds_wed_marginalize_frame(frame)"""
    n = int(snap["counts"][0])
    ip, ir = survivors(snap, point_flag, select, mutate, frame)
    out = {k: dict(v) for k, v in snap.items() if isinstance(v, dict)}
    for group, names in PER_RESIDUAL:
        for k in (names or list(snap[group])):
            rows = snap[group][k]
            if mutate == "solver_rows_left_behind" and k in ("is_linearized", "res_toZeroF"):
                out[group][k] = rows[:len(ir)]
            else:
                out[group][k] = rows[ir]
    for group, names in PER_POINT:
        for k in (names or list(snap[group])):
            out[group][k] = snap[group][k][ip]
    new_index = np.full(n, -1, np.int64)
    new_index[ip] = np.arange(len(ip))
    old_point = snap["rows"]["point"][ir]
    point = old_point if mutate == "points_not_renumbered" else new_index[old_point]
    out["rows"]["point"] = point.astype(np.int32)
    first = np.zeros(len(ip) + 1, np.int32)
    if mutate == "stale_res_first":
        first[:] = snap["rows"]["res_first"][np.append(ip, n)]
    else:
        first[1:] = np.cumsum(np.bincount(new_index[old_point][new_index[old_point] >= 0], minlength=len(ip)))
    out["rows"]["res_first"] = first
    if frame is not None:
        t, h = out["rows"]["target"], out["rows"]["host"]
        out["rows"]["target"] = t if mutate == "targets_not_renumbered" else (t - (t > frame)).astype(np.int32)
        out["rows"]["host"] = h if mutate == "hosts_not_renumbered" else (h - (h > frame)).astype(np.int32)
    out["counts"] = np.array([len(ip), len(ir)], np.int32)
    out["per_host"] = np.bincount(out["rows"]["host"], minlength=8).astype(np.int32)
    return out


def after_set_state(snap, scale_idepth=1.0):
    """a snapshot after eds_wed_set_state: priorF, is_linearized and res_toZeroF stay; deltaF comes from the inverse depths
    (setDeltaF, in fp32); the L sums, the steps, resApprox are cleared and no backup holds"""
    out = {k: (dict(v) if isinstance(v, dict) else v) for k, v in snap.items()}
    for k in ("resApprox", "lf", "step"):
        out["state"][k] = np.zeros_like(snap["state"][k])
    inv = np.float32(1.0) / np.float32(scale_idepth)
    out["rows"]["deltaF"] = (inv * snap["state"]["idepth_scaled"] - inv * snap["rows"]["idepth_zero_scaled"]).astype(np.float32)
    out["rows"]["idepth_backup"] = np.zeros_like(snap["rows"]["idepth_backup"])
    return out


def tables(snap):
    """what eds_win_set_points / eds_win_set_residuals take, from a snapshot: a fresh window with the same points and residuals"""
    r, p, s = snap["rows"], snap["residuals"], snap["state"]
    return dict(points=(r["host"], r["uv"], r["color"], r["weights"], s["idepth_scaled"], r["idepth_zero_scaled"]),
                residuals=(r["point"], r["target"], p["state"], p["energy"]))


# ---- marginalizeFrame's arithmetic: the header's nine steps, every dot product an explicit loop -----------------------------------------

def inverse8(a, mutate=None):
    """the stated LU with partial pivoting and the substitutions on the columns of I; None for a zero pivot or a result not finite"""
    a = np.array(a, dtype=np.float64).reshape(8, 8).copy()
    perm = list(range(8))
    for k in range(8):
        p, best = k, abs(a[k, k])
        for r in range(k + 1, 8):
            v = abs(a[r, k])
            if v > best or (mutate == "pivot_highest_on_tie_or_none" and v >= best):
                best, p = v, r
        if not a[p, k] != 0.0:
            return None
        if p != k:
            a[[k, p]] = a[[p, k]]
            perm[k], perm[p] = perm[p], perm[k]
        for r in range(k + 1, 8):
            l = a[r, k] / a[k, k]
            a[r, k] = l
            for c in range(k + 1, 8):
                a[r, c] = a[r, c] - l * a[k, c]
    hpi = np.zeros((8, 8))
    for e in range(8):
        y, x = np.zeros(8), np.zeros(8)
        for i in range(8):
            s = np.float64(0.0)
            for j in (range(i) if mutate != "sum_descending" else reversed(range(i))):
                s = s + a[i, j] * y[j]
            y[i] = (1.0 if perm[i] == e else 0.0) - s
        for i in reversed(range(8)):
            s = np.float64(0.0)
            for j in (range(i + 1, 8) if mutate != "sum_descending" else reversed(range(i + 1, 8))):
                s = s + a[i, j] * x[j]
            x[i] = (y[i] - s) / a[i, i]
        if not np.isfinite(x).all():
            return None
        hpi[:, e] = x
    return hpi


def permutation(N, frame, mutate=None):
    io, nd = 4 + 8 * frame, N - 8
    if mutate == "permutation_off_by_one_block":
        io = 4 + 8 * ((frame + 1) % ((N - 4) // 8))
    return np.array([i if i < io else i + 8 if i < nd else io + (i - nd) for i in range(N)])


def marginalize_frame(HM, bM, frame, prior, delta_prior, mutate=None):
    """(HM', bM') by the header's steps, or None where it says EDS_ERR_NOT_USABLE"""
    with np.errstate(all="ignore"):
        bM = np.asarray(bM, dtype=np.float64)
        N = len(bM)
        nd = N - 8
        P = permutation(N, frame, mutate)
        H = np.asarray(HM, dtype=np.float64).reshape(N, N)[np.ix_(P, P)].copy()
        b = bM[P].copy()
        if mutate != "prior_not_added":
            for k in range(8):
                H[nd + k, nd + k] = H[nd + k, nd + k] + prior[k]
                b[nd + k] = b[nd + k] + prior[k] * delta_prior[k]
        S = np.sqrt(np.abs(np.diag(H)) + 10.0)
        SI = 1.0 / S
        H = (SI[:, None] * H) * SI[None, :]
        b = SI * b
        hpi = inverse8(H[nd:, nd:], mutate)
        if hpi is None:
            return None
        bli = np.zeros((nd, 8))
        for i in range(nd):
            for k in range(8):
                s = np.float64(0.0)
                for j in (range(8) if mutate != "sum_descending" else reversed(range(8))):
                    s = s + H[nd + j, i] * hpi[j, k]
                bli[i, k] = s
        T, tb = H[:nd, :nd].copy(), b[:nd].copy()
        acc, accb = np.zeros((nd, nd)), np.zeros(nd)
        for k in (range(8) if mutate != "sum_descending" else reversed(range(8))):   # the sums over k from 0.0 in ascending k, for every (i, j) at once
            acc = acc + bli[:, k][:, None] * H[nd + k, :nd][None, :]
            accb = accb + bli[:, k] * b[nd + k]
        T, tb = T - acc, tb - accb
        U = S[:nd] if mutate != "unscale_by_SI" else SI[:nd]
        T = (U[:, None] * T) * U[None, :]
        tb = U * tb
        out = 0.5 * (T + T.T) if mutate != "missing_symmetrisation" else T
        if not (np.isfinite(out).all() and np.isfinite(tb).all()):
            return None
        return out, tb


def marginalize_frame_extended(HM, bM, frame, prior, delta_prior):
    """the Schur complement in numpy.longdouble (scaled by its own S, Gauss-Jordan with partial pivoting on the 8 x 8), and what the
    bound of DESIGN 21 is built from: (HM', bM', S, |A|, |B|^T |hpi| |B|, |b_head|, |B|^T |hpi| |b_tail|, cond of the scaled 8 x 8)"""
    ld = np.longdouble
    bM = np.asarray(bM, dtype=ld)
    N = len(bM)
    nd = N - 8
    P = permutation(N, frame)
    H = np.asarray(HM, dtype=ld).reshape(N, N)[np.ix_(P, P)].copy()
    b = bM[P].copy()
    H[np.arange(nd, N), np.arange(nd, N)] += np.asarray(prior, dtype=ld)
    b[nd:] += np.asarray(prior, dtype=ld) * np.asarray(delta_prior, dtype=ld)
    S = np.sqrt(np.abs(np.diag(H)) + ld(10))
    Hs, bs = H / S[:, None] / S[None, :], b / S
    C = Hs[nd:, nd:].copy()
    aug = np.concatenate([C, np.eye(8, dtype=ld)], axis=1)
    for k in range(8):
        p = k + int(np.argmax(np.abs(aug[k:, k])))
        aug[[k, p]] = aug[[p, k]]
        aug[k] = aug[k] / aug[k, k]
        for r in range(8):
            if r != k:
                aug[r] = aug[r] - aug[r, k] * aug[k]
    hpi = aug[:, 8:]
    B = Hs[nd:, :nd]
    T = Hs[:nd, :nd] - B.T @ hpi @ B
    tb = bs[:nd] - B.T @ hpi @ bs[nd:]
    T = 0.5 * (T + T.T)
    Sh = S[:nd]
    W = np.abs(B).T @ np.abs(hpi) @ np.abs(B)
    wb = np.abs(B).T @ np.abs(hpi) @ np.abs(bs[nd:])
    cond = float(np.linalg.cond(C.astype(np.float64)))
    return T * Sh[:, None] * Sh[None, :], tb * Sh, Sh, np.abs(Hs[:nd, :nd]), W, np.abs(bs[:nd]), wb, cond


def frame_bound(Sh, A, W, bh, wb, cond):
    """DESIGN 21's componentwise bound on |HM' - exact| and |bM' - exact|, in units of 2^-53"""
    u = 2.0 ** -53
    c_prod = 26.0 + 16.0 * cond
    return (u * Sh[:, None] * Sh[None, :] * (8.0 * A + c_prod * W)).astype(np.float64), (u * Sh * (8.0 * bh + c_prod * wb)).astype(np.float64)


# ---- activated points enter -----------------------------------------------------------------------------------------------------------

INSERT_MUTATIONS = ("activated_first", "appended_at_the_end", "new_state_in", "idepth_zero_left_zero")


def insert(snap, points, residuals, mutate=None):
    """the snapshot after eds_wed_insert_activated: `points`, `residuals` are what Activation.window_tables() returns (one row per
    activated point in (host, index) order, one residual per IN target in ascending target).  Per host the window's own points first,
    then the host's activated ones: a stable sort of the concatenation by host.  New rows are what eds_win_set_points /
    eds_win_set_residuals leave (state IN, energy 0, new state OUTLIER, everything else 0)."""
    n, m = int(snap["counts"][0]), int(snap["counts"][1])
    K, R = len(points["host"]), len(residuals["point"])
    host_all = np.concatenate([snap["rows"]["host"], points["host"]]).astype(np.int32)
    if mutate == "activated_first":
        order = np.lexsort((np.concatenate([np.ones(n), np.zeros(K)]), host_all))
    elif mutate == "appended_at_the_end":
        order = np.arange(n + K)
    else:
        order = np.argsort(host_all, kind="stable")               # source row (old: < n, new: n + k) of every merged point
    new_index = np.empty(n + K, np.int64)
    new_index[order] = np.arange(n + K)
    out = {k: dict(v) for k, v in snap.items() if isinstance(v, dict)}

    def merged(old, new_rows):
        return np.concatenate([old, new_rows.astype(old.dtype).reshape((len(new_rows),) + old.shape[1:])])

    zeros = lambda a, k: np.zeros((k,) + a.shape[1:], a.dtype)      # noqa: E731
    idz = points["idepth_zero_scaled"] if mutate != "idepth_zero_left_zero" else np.zeros(K, np.float32)
    given_p = dict(host=points["host"], uv=points["uv"], color=points["color"], weights=points["weights"], idepth_scaled=points["idepth_scaled"],
                   idepth_zero_scaled=idz)
    for group, names in PER_POINT:
        for k in (names or list(snap[group])):
            a = snap[group][k]
            out[group][k] = merged(a, given_p[k] if k in given_p else zeros(a, K))[order]
    # residuals: sort all (old and new) by their point's merged index, stable, new ones of a point in the order given
    point_all = np.concatenate([new_index[snap["rows"]["point"]], new_index[n + residuals["point"]]])
    rorder = np.argsort(point_all, kind="stable")
    given_r = dict(target=residuals["target"], state=residuals["state"], energy=residuals["energy"], new_energy=residuals["energy"],
                   new_state=np.full(R, 2 if mutate != "new_state_in" else 0, np.int32))
    for group, names in PER_RESIDUAL:
        for k in (names or list(snap[group])):
            a = snap[group][k]
            out[group][k] = merged(a, given_r[k] if k in given_r else zeros(a, R))[rorder]
    out["rows"]["point"] = point_all[rorder].astype(np.int32)
    first = np.zeros(n + K + 1, np.int32)
    first[1:] = np.cumsum(np.bincount(point_all, minlength=n + K))
    out["rows"]["res_first"] = first
    out["counts"] = np.array([n + K, m + R], np.int32)
    out["per_host"] = np.bincount(out["rows"]["host"], minlength=8).astype(np.int32)
    return out
