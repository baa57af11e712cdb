"""A literal numpy statement of include/eds_hip_winflag.h: the history columns (per point num_good, max_rel_baseline, last_target[2],
last_state[2]; per residual is_new), what every edit of include/eds_hip_winedit.h does to them, makeKeyFrame's residuals towards a
new keyframe, and the history half of the fixLinearization pass.  Plain loops over points and runs; fp32 where the header says fp32.

A history is a dict of the five arrays.  `mutate` names one deliberate mistake (MUTATIONS): tests/test_winflag_oracle.py shows that the
restatement under g++ tells every one of them from the statement."""
import numpy as np

IN, OOB, OUTLIER = 0, 1, 2
f32 = np.float32
COLUMNS = ("num_good", "max_rel_baseline", "last_target", "last_state", "is_new")
MUTATIONS = ("order_1_before_0", "no_shift", "shift_keeps_state", "forget_keeps_target", "forget_clears_state", "no_decrement", "decrement_from_frame",
             "new_residual_first_in_run", "host_gets_a_residual", "clear_is_new_ignored", "is_new_ignored", "inactive_counted", "maximum_is_last",
             "activated_latest_is_f_minus_2", "new_residual_not_new")


def defaults(n, m):
    return dict(num_good=np.zeros(n, np.int32), max_rel_baseline=np.zeros(n, f32), last_target=np.full((n, 2), -1, np.int32),
                last_state=np.full((n, 2), OOB, np.int32), is_new=np.ones(m, np.int32))


def copy(hist):
    return {k: np.array(hist[k], copy=True) for k in COLUMNS}


def runs(point, n):
    """res_first: point p's residuals are res_first[p] .. res_first[p + 1] - 1"""
    first = np.zeros(n + 1, np.int64)
    for p in point:
        first[p + 1] += 1
    return np.cumsum(first)


def remove_residuals(hist, point, target, keep_r, mutate=None):
    """the residuals with keep_r == 0 leave, every point stays"""
    h = copy(hist)
    for r in range(len(point)):
        if keep_r[r]:
            continue
        for k in range(2):
            if h["last_target"][point[r], k] == target[r]:
                if mutate != "forget_keeps_target":
                    h["last_target"][point[r], k] = -1
                if mutate == "forget_clears_state":
                    h["last_state"][point[r], k] = OOB
    h["is_new"] = h["is_new"][np.flatnonzero(np.asarray(keep_r) != 0)]
    return h


def remove_points(hist, point, keep_p):
    """the points with keep_p == 0 leave with all their residuals; a survivor's history moves with it"""
    kp = np.flatnonzero(np.asarray(keep_p) != 0)
    h = {k: np.array(hist[k][kp], copy=True) for k in COLUMNS[:4]}
    h["is_new"] = np.array(hist["is_new"][np.asarray(keep_p)[point] != 0], copy=True)
    return h


def marginalize_frame(hist, point, target, frame, mutate=None):
    """every residual towards `frame` leaves, then the frames above it are one lower"""
    h = remove_residuals(hist, point, target, np.asarray(target) != frame, mutate)
    lt = h["last_target"]
    for p in range(len(lt)):
        for k in range(2):
            above = lt[p, k] >= frame if mutate == "decrement_from_frame" else lt[p, k] > frame
            if above and mutate != "no_decrement":
                lt[p, k] -= 1
    return h


def activated(hist_rows, target_mask, F, mutate=None):
    """the history of activated points whose fit left residuals towards the targets of target_mask (eds_act_get_activated)"""
    K = len(target_mask)
    h = defaults(K, 0)
    for q in range(K):
        for k in range(2):
            f = F - 1 - k - (1 if mutate == "activated_latest_is_f_minus_2" else 0)
            if f >= 0 and (int(target_mask[q]) >> f) & 1:
                h["last_target"][q, k], h["last_state"][q, k] = f, IN
    return h


def insert_frame_residuals(hist, host, point, target, frame, mutate=None):
    """makeKeyFrame's loop: (point, target, map new -> old with -1 for a new row, history) after it"""
    n, m = len(host), len(point)
    first = runs(point, n)
    h = copy(hist)
    new_point, new_target, new_map, is_new = [], [], [], []
    for p in range(n):
        run = list(range(first[p], first[p + 1]))
        need = (host[p] != frame or mutate == "host_gets_a_residual") and not any(target[r] == frame for r in run)
        rows = [(p, target[r], r, h["is_new"][r]) for r in run]
        if need:
            new = (p, frame, -1, 0 if mutate == "new_residual_not_new" else 1)
            rows = [new] + rows if mutate == "new_residual_first_in_run" else rows + [new]
            if mutate != "no_shift":
                h["last_target"][p, 1] = h["last_target"][p, 0]
                if mutate != "shift_keeps_state":
                    h["last_state"][p, 1] = h["last_state"][p, 0]
            h["last_target"][p, 0], h["last_state"][p, 0] = frame, IN
        for a, b, c, d in rows:
            new_point.append(a), new_target.append(b), new_map.append(c), is_new.append(d)
    h["is_new"] = np.array(is_new, np.int32).reshape(-1)
    assert len(new_point) <= m + n
    return np.array(new_point, np.int32).reshape(-1), np.array(new_target, np.int32).reshape(-1), np.array(new_map, np.int32).reshape(-1), h


def rel_baseline(pc, u, v, idepth):
    """relBS of one residual: pc is the 27-float (host, target) record; every operation fp32, rows summed left to right"""
    with np.errstate(all="ignore"):
        K, t, one = pc[:9], pc[9:12], f32(1.0)
        inf = [f32(f32(f32(K[3 * i] * u) + f32(K[3 * i + 1] * v)) + f32(K[3 * i + 2] * one)) for i in range(3)]
        ptp = [f32(inf[i] + f32(t[i] * idepth)) for i in range(3)]
        dx = f32(f32(inf[0] / inf[2]) - f32(ptp[0] / ptp[2]))
        dy = f32(f32(inf[1] / inf[2]) - f32(ptp[1] / ptp[2]))
        return f32(0.01 * np.float64(np.sqrt(f32(f32(dx * dx) + f32(dy * dy)), dtype=f32)))


def apply_fixed(hist, host, uv, idepth, point, target, state, active, precalc, F, clear_is_new, mutate=None):
    """the history after the pass, given the tables as applyRes(true) left them: (history, counts[3], what happened)"""
    n = len(host)
    first = runs(point, n)
    h = copy(hist)
    pc = np.asarray(precalc, f32).reshape(F * F, 27)
    counts = np.zeros(3, np.int32)
    seen = dict(hit0=0, hit1=0, miss=0, raised=0, not_raised=0, good=0, skipped_old=0, skipped_inactive=0)
    for p in range(n):
        for r in range(first[p], first[p + 1]):
            new = h["is_new"][r] != 0 or mutate == "is_new_ignored"
            on = active[r] != 0 or mutate == "inactive_counted"
            if on and new:
                rel = rel_baseline(pc[host[p] * F + target[r]], f32(uv[p][0]), f32(uv[p][1]), f32(idepth[p]))
                wins = rel > h["max_rel_baseline"][p] or mutate == "maximum_is_last"
                if wins:
                    h["max_rel_baseline"][p] = rel
                seen["raised" if wins else "not_raised"] += 1
                h["num_good"][p] += 1
                seen["good"] += 1
            else:
                seen["skipped_inactive" if new else "skipped_old"] += 1
            order = (1, 0) if mutate == "order_1_before_0" else (0, 1)
            if h["last_target"][p, order[0]] == target[r]:
                h["last_state"][p, order[0]] = state[r]
                seen["hit%d" % order[0]] += 1
            elif h["last_target"][p, order[1]] == target[r]:
                h["last_state"][p, order[1]] = state[r]
                seen["hit%d" % order[1]] += 1
            else:
                seen["miss"] += 1
            counts[state[r]] += 1
    if clear_is_new and mutate != "clear_is_new_ignored":
        h["is_new"][:] = 0
    return h, counts, seen


# ---- flagPointsForRemoval ----------------------------------------------------------------------------------------------------------------
KEEP, MARGINALIZE, DROP = 0, 1, 2
PARAMS = dict(min_good_active_res_for_marg=3, min_good_res_for_marg=4, min_idepth_h_marg=50.0)
FLAG_MUTATIONS = ("oob_size_gt", "oob_good_ge", "oob_rest_le", "oob_last0_outlier", "oob_size_le_2", "oob_either_outlier", "oob_counts_every_state",
                  "inlier_size_gt", "inlier_good_gt", "hessian_ge", "idepth_le", "host_bit_ignored", "empty_run_kept", "only_empty_ignored")


def is_oob(size, good, last_state, run_states, run_targets, frames_to_marg, prm, mutate=None, seen=None):
    """PointHessian::isOOB, literally; `seen` counts which return was taken"""
    A, G = prm["min_good_active_res_for_marg"], prm["min_good_res_for_marg"]
    vis = 0
    for st, t in zip(run_states, run_targets):
        if st != IN and mutate != "oob_counts_every_state":
            continue
        if (frames_to_marg >> int(t)) & 1:
            vis += 1
    c1 = size > A if mutate == "oob_size_gt" else size >= A
    c2 = good >= G + 10 if mutate == "oob_good_ge" else good > G + 10
    c3 = size - vis <= A if mutate == "oob_rest_le" else size - vis < A
    taken = None
    if c1 and c2 and c3:
        taken = "oob_true_few_left"
    elif last_state[0] == (OUTLIER if mutate == "oob_last0_outlier" else OOB):
        taken = "oob_true_last_oob"
    elif (size <= 2 if mutate == "oob_size_le_2" else size < 2):
        taken = "oob_false_short"
    elif (last_state[0] == OUTLIER or last_state[1] == OUTLIER) if mutate == "oob_either_outlier" else (last_state[0] == OUTLIER and last_state[1] == OUTLIER):
        taken = "oob_true_two_outliers"
    else:
        taken = "oob_false"
    if seen is not None:
        seen[taken] = seen.get(taken, 0) + 1
    return taken.startswith("oob_true")


def flag_points(hist, host, idepth, point, target, state, idepth_hessian, frames_to_marg, only_empty=False, prm=None, mutate=None):
    """(fates, counts[27]: kept, marginalised, dropped and the same per host, the candidates that were re-linearized, what happened)"""
    prm = dict(PARAMS, **(prm or {}))
    n = len(host)
    first = runs(point, n)
    fates, cand, seen = np.zeros(n, np.int32), np.zeros(n, np.int32), {}
    hit = lambda k: seen.__setitem__(k, seen.get(k, 0) + 1)      # noqa: E731
    for p in range(n):
        r0, r1 = int(first[p]), int(first[p + 1])
        size = r1 - r0
        if only_empty and mutate != "only_empty_ignored":
            fates[p] = DROP if size == 0 else KEEP
            continue
        negative = f32(idepth[p]) <= 0 if mutate == "idepth_le" else f32(idepth[p]) < 0
        if negative or (size == 0 and mutate != "empty_run_kept"):
            fates[p] = DROP
            hit("negative_idepth" if negative else "empty_run")
            continue
        oob = is_oob(size, hist["num_good"][p], hist["last_state"][p], state[r0:r1], target[r0:r1], frames_to_marg, prm, mutate, seen)
        flagged = bool((frames_to_marg >> int(host[p])) & 1) and mutate != "host_bit_ignored"
        if oob or flagged:
            if flagged and not oob:
                hit("host_flagged_not_oob")
            A, G = prm["min_good_active_res_for_marg"], prm["min_good_res_for_marg"]
            inlier = (size > A if mutate == "inlier_size_gt" else size >= A) and (hist["num_good"][p] > G if mutate == "inlier_good_gt" else hist["num_good"][p] >= G)
            if inlier:
                cand[p] = 1
                big = f32(idepth_hessian[p]) >= f32(prm["min_idepth_h_marg"]) if mutate == "hessian_ge" else f32(idepth_hessian[p]) > f32(prm["min_idepth_h_marg"])
                fates[p] = MARGINALIZE if big else DROP
                hit("hessian_above" if big else "hessian_at_or_below")
            else:
                fates[p] = DROP
                hit("not_inlier")
        else:
            fates[p] = KEEP
    counts = np.zeros(27, np.int32)
    for p in range(n):
        counts[fates[p]] += 1
        counts[3 + 3 * host[p] + fates[p]] += 1
    return fates, counts, cand, seen
