# -*- coding: utf-8 -*-
"""The causal running mean / variance normalisation restated in numpy: a plain loop over frames on
np.float64 scalars, every operation one IEEE operation in the order the rule writes them.  Not used by the product."""
import numpy as np


def fresh_state(D):
    """(S [D], Q [D], c): the sums and the count of the frames they hold, all zero."""
    return np.zeros(D, dtype=np.float64), np.zeros(D, dtype=np.float64), 0


def running_norm(x, mean, std, prior_frames=100, min_std=0.1, dtype=np.float64, state=None):
    """x [T, D] raw features -> (y [T, D] of `dtype`, state after the last frame).  The raw value is first rounded to
    `dtype` (an explicit np.float32 round trip for fp32 batches), as the resident batch holds it; `state` carries
    (S, Q, c) from an earlier call, None starts from zero."""
    dtype = np.dtype(dtype).type
    x = np.asarray(x)
    T, D = x.shape
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    P, phi = np.float64(prior_frames), np.float64(min_std)
    S, Q, c = fresh_state(D) if state is None else (state[0].copy(), state[1].copy(), int(state[2]))
    y = np.empty((T, D), dtype=dtype)
    ps2 = [(P * std[k]) * std[k] for k in range(D)]                   # the host forms these once, in this order
    fl2 = [(phi * std[k]) * (phi * std[k]) for k in range(D)]
    for t in range(T):
        c += 1
        n = P + np.float64(c)
        for k in range(D):
            r = np.float64(dtype(x[t, k]))
            d = r - mean[k]
            S[k] = S[k] + d
            Q[k] = Q[k] + d * d
            a = S[k] / n
            v = (ps2[k] + Q[k]) / n - a * a
            sd = np.sqrt(max(v, fl2[k]))
            y[t, k] = dtype((d - a) / sd)
    return y, (S, Q, c)
