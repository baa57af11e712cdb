"""gridMaxSelection and makePixelStatus as the reference writes them (src/init/CoarseInitializer.h, lines quoted as H:n), in numpy scalars:
every value a np.float32, every loop in the reference's order, the global ``sparsityFactor`` (src/utils/settings.cpp:212) passed in and
returned.  Slow and plain on purpose: tests/test_inisetup_oracle.py holds csrc/eds_inisetup.hpp under g++ to it, and
tests/test_inisetup_gpu.py holds the device to that build."""
import numpy as np

F = np.float32
MIN_USE_GRAD_PIXSEL = F(10)                  # H:81


def grid_max_selection(grads, pot, th_fac, ties=None):
    """H:164-240 (the templates H:84-161 are the same text).  grads: h x w x {colour, dx, dy} float32.  Returns (map h x w uint8,
    numGood).  `ties`, a list, receives one entry per cell whose winning score in some direction is reached by two or more pixels."""
    h, w = grads.shape[:2]
    g = grads.reshape(h * w, 3)
    map_out = np.zeros(h * w, np.uint8)                                          # H:167
    th_fac = F(th_fac)
    num_good = 0
    for y in range(1, h - pot, pot):                                             # H:170
        for x in range(1, w - pot, pot):                                         # H:172
            best_id = [-1, -1, -1, -1]                                           # H:174-177
            best = [F(0), F(0), F(0), F(0)]                                      # H:179
            reached = [1, 1, 1, 1]
            o = x + y * w                                                        # H:181
            for dx in range(pot):                                                # H:182
                for dy in range(pot):                                            # H:183
                    idx = dx + dy * w                                            # H:185
                    g1, g2 = g[o + idx, 1], g[o + idx, 2]
                    sqgd = F(g1 * g1) + F(g2 * g2)                               # H:187
                    th = F(F(th_fac * MIN_USE_GRAD_PIXSEL) * F(0.75))            # H:188
                    if sqgd > F(th * th):                                        # H:190
                        with np.errstate(invalid="ignore"):                      # inf - inf: a NaN score never wins
                            scores = (np.abs(g1), np.abs(g2), np.abs(F(g1 - g2)), np.abs(F(g1 + g2)))     # H:192-201
                        for k in range(4):
                            if scores[k] > best[k]:
                                best[k], best_id[k], reached[k] = scores[k], idx, 1
                            elif scores[k] == best[k] and best_id[k] >= 0:
                                reached[k] += 1
            for k in range(4):                                                   # H:208-235
                if best_id[k] >= 0:
                    if not map_out[o + best_id[k]]:
                        num_good += 1
                    map_out[o + best_id[k]] = 1
            if ties is not None and any(best_id[k] >= 0 and reached[k] > 1 for k in range(4)):
                ties.append((x, y))
    return map_out.reshape(h, w), num_good


def make_pixel_status(grads, desired_density, recs_left, th_fac, sparsity, trace=None):
    """H:243-297.  Returns (map, numGoodPoints, passes, sparsityFactor afterwards).  `trace`, a list, receives (sparsityFactor, THFac,
    numGoodPoints) of every pass."""
    th_fac = F(th_fac)
    passes = 0
    while True:
        if sparsity < 1:                                                         # H:245
            sparsity = 1
        status, num_good = grid_max_selection(grads, sparsity, th_fac)           # H:250-261
        passes += 1
        if trace is not None:
            trace.append((sparsity, float(th_fac), num_good))
        with np.errstate(divide="ignore"):
            quotia = F(num_good) / F(desired_density)                            # H:268
            new_sparsity = int(F(F(F(sparsity) * np.sqrt(quotia)) + F(0.7)))     # H:270
            if new_sparsity < 1:                                                 # H:273
                new_sparsity = 1
            old_th_fac = th_fac                                                  # H:276
            if new_sparsity == 1 and sparsity == 1:                              # H:277
                th_fac = F(0.5)
            stop = ((abs(new_sparsity - sparsity) < 1 and th_fac == old_th_fac) or
                    (float(quotia) > 0.8 and float(F(1) / quotia) > 0.8) or recs_left == 0)      # H:280-282
        sparsity = new_sparsity                                                  # H:287, H:294
        if stop:
            return status, num_good, passes, sparsity
        recs_left -= 1                                                           # H:295
