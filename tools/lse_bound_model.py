#!/usr/bin/env python3
"""CPU model of the two fp64 log-sum-exp epilogues of the matrix-core likelihood kernel.

The kernel's default epilogue takes the mixture's log-sum-exp against a reference point that is known when the model is
packed, mh_s = max C_g over the switched-on components of state s (a_g(x) <= C_g for diagonal Gaussians), instead of
the per-frame maximum:

    y_g = K (a_g - mh_s) <= 0,   s = sum_g 2^(y_g / 128),   nll = -(K mh_s + K ln s) / K,   K = 128 / ln 2.

Its result is taken only where s >= thr_s; everything else is redone in the max-shifted form.  This tool models both
forms with numpy, for mixtures of one tile per state (M <= 16; larger mixtures keep the max-shifted form in the
kernel): the component log-densities in long double; the bound form with its terms 2^(y/128) ROUNDED TO fp64 (gradual
underflow and flush to zero included -- the one place where the reference point matters), the sum in fp64, the logarithm
in long double; the redo with the maximum, the shifted terms, their sum and the final additions in fp64, and the
reference's +inf rule on max(y) + K mh_s.  A state without a switched-on finite component is packed as the kernel
packs it (NaN constants stay only when every slot of the padded mixture is NaN).  Against the exact long-double
log-sum-exp it reports

  * the largest relative error of the result: the bound form where the guard lets it through, the redo elsewhere,
  * whether anything comes out +inf (the compat rule: largest term below ln 2^-1075) or NaN where the exact form does
    not, or the other way round,
  * the share of frames x states, and of 32-frame blocks, that take the redo.

    python tools/lse_bound_model.py                 # bench.synth_workload(1002, 200) and the edge models
    python tools/lse_bound_model.py --frames 4000   # fewer frames of the bench workload

tests/test_lse_bound_host.py runs the same functions on small shapes.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
K = LD(128) / np.log(LD(2))
THR_PLAIN = 2.0 ** -900
COMPAT_BELOW = float(LD(-1075) * np.log(LD(2)))          # ln 2^-1075, nats


def pack(means, vars_, w):
    """C[S,M] (long double, -inf: switched off), mh[S] (0 where no component is on), any_on[S]"""
    means, vars_, w = (np.asarray(a, dtype=np.float64) for a in (means, vars_, w))
    S, M, D = means.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        logw = np.log(w.astype(LD))
        C = logw - LD(0.5) * (D * np.log(LD(2) * LD(np.pi)) + np.sum(np.log(vars_.astype(LD)), axis=2))
    on = np.isfinite(C)
    any_on = on.any(axis=1)
    # no switched-on finite component: the max-shifted form's maximum drops NaN operands, so the state is +inf as soon as
    # one slot of the padded mixture is OFF, and NaN only when every slot is NaN (gh_pack_lse_state)
    for st in np.nonzero(~any_on)[0]:
        if not (np.isnan(C[st]).all() and m_pad_of(M) == M):
            C[st] = -np.inf
    mh = np.where(any_on, np.where(on, C, -np.inf).max(axis=1), 0).astype(LD)
    return C, mh, any_on


def thresholds(mh, any_on, M_pad, compat):
    """thr[S] as gh_lse_state_of packs it and the kernel stages it: 2^-900, in compat mode also 2 M_pad 2^(-1075 - mh/ln2)"""
    thr = np.full(len(mh), THR_PLAIN)
    if compat:
        ex = (LD(COMPAT_BELOW) - mh) / np.log(LD(2))
        with np.errstate(over="ignore"):
            t = np.where(ex > 1000, np.inf, np.where(ex < -1060, 0.0, (2.0 * M_pad) * np.exp2(np.clip(ex, -1100, 1001)))).astype(np.float64)
        thr = np.maximum(thr, t)
    return np.where(any_on, thr, np.inf)


def m_pad_of(M):
    if M <= 16:
        p = 1
        while p < M:
            p <<= 1
        return p
    return (M + 15) & ~15


def component_logdens(X, means, vars_, C):
    """a[N,S,M] in long double (mean-centred form: no cancellation)"""
    X = np.asarray(X, dtype=LD)
    dx = X[:, None, None, :] - np.asarray(means, dtype=LD)[None]
    return C[None] - LD(0.5) * np.sum(dx * dx / np.asarray(vars_, dtype=LD)[None], axis=3)


def evaluate(X, means, vars_, w, compat=True):
    """dict of [N,S] arrays: exact (long double nll, the compat rule applied), fast (the bound form's fp64 result), s
    (its sum), cold (the guard sends the cell to the redo), plus thr[S] and mh[S]"""
    C, mh, any_on = pack(means, vars_, w)
    M = C.shape[1]
    thr = thresholds(mh, any_on, m_pad_of(M), compat)
    a = component_logdens(X, means, vars_, C)                                     # [N,S,M]
    amax = a.max(axis=2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        exact = -(amax + np.log(np.exp(a - amax[..., None]).sum(axis=2)))
        exact = np.where(np.isnan(amax), np.nan, np.where(np.isfinite(amax), exact, np.inf))     # (a NaN constant poisons its state)
        if compat:
            exact = np.where(amax < LD(COMPAT_BELOW), np.inf, exact)
        y = (a - mh[None, :, None]) * K                                           # scaled, <= 0
        terms = np.exp2(y / 128).astype(np.float64)                               # fp64: subnormals round, then flush to 0
        s = terms.sum(axis=2)
        fast = (-(mh[None] * K + K * np.log(s.astype(LD))) / K).astype(np.float64)
        cold = s < thr[None]
        # the redo, in fp64 on the same shifted accumulators: max, shifted terms, sum, logarithm, K mh added last
        y64 = np.where(np.isneginf(y), -1e300, y).astype(np.float64)
        m64 = np.fmax.reduce(y64, axis=2)                                         # (v_max_f64 drops a NaN operand)
        s64 = np.exp2((y64 - m64[..., None]) / 128.0).sum(axis=2)
        kmh = (mh * K).astype(np.float64)
        redo = -((m64 + float(K) * np.log(s64)) + kmh[None]) / float(K)
        below = float(LD(COMPAT_BELOW) * K) if compat else -1e299
        redo = np.where(m64 + kmh[None] < below, np.inf, redo)
    result = np.where(cold, redo, fast)
    return dict(exact=exact, fast=fast, redo=redo, result=result, s=s, cold=cold, thr=thr, mh=mh, amax=amax)


def check(res, compat=True):
    """(largest relative error of the results -- the bound form where the guard accepts it, the fp64 redo elsewhere --,
    number of cells whose +inf / NaN differs from the exact form's, share of cells on the redo, share of 32-frame blocks
    with a cell on the redo)"""
    ok = ~res["cold"]
    exact, fast = res["exact"], res["fast"]
    wrong_inf = int(np.sum(ok & np.isinf(exact))) + int(np.sum(ok & (np.isnan(exact) != np.isnan(fast))))
    fin = ok & np.isfinite(exact)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs((fast.astype(LD) - exact) / exact)
    worst = float(rel[fin].max()) if fin.any() else 0.0
    N = ok.shape[0]
    blocks = [res["cold"][i:i + 32].any() for i in range(0, N, 32)]
    # the redo's own results: +inf / NaN exactly where the exact form has them, finite values within the same bound
    redone, out = res["cold"], res["result"]
    if not (np.array_equal(np.isinf(out[redone]), np.isinf(exact[redone])) and np.array_equal(np.isnan(out[redone]), np.isnan(exact[redone]))):
        wrong_inf += 1
    finr = redone & np.isfinite(exact)
    with np.errstate(invalid="ignore", divide="ignore"):
        relr = np.abs((out.astype(LD) - exact) / exact)
    if finr.any():
        worst = max(worst, float(relr[finr].max()))
    return worst, wrong_inf, float(res["cold"].mean()), float(np.mean(blocks))


def edge_models(seed=0):
    """(name, X, means, vars, w): the shapes and corners of tests/test_gpu_loglik_bound.py"""
    rng = np.random.default_rng(seed)
    out = []
    for S, M, D, N in ((2, 2, 3, 17), (5, 4, 3, 33), (7, 8, 39, 33), (3, 16, 39, 17), (4, 3, 3, 17)):
        means = rng.normal(size=(S, M, D))
        vars_ = rng.uniform(0.5, 1.5, size=(S, M, D))
        w = rng.dirichlet(np.ones(M), size=S)
        X = rng.normal(size=(N, D)) * 1.5
        out.append(("random S%d M%d D%d" % (S, M, D), X, means, vars_, w))
        # frames moved away from every mean: around the guard (~ -620 nats), between it and -745, beyond, far beyond
        far = X.copy()
        for i, r in enumerate(np.linspace(20.0, 60.0, N)):
            far[i] = means[0, 0] + r * np.sqrt(2.0 / D) * np.sign(rng.normal(size=D))
        far[-1] *= 40.0
        out.append(("far frames S%d M%d D%d" % (S, M, D), far, means, vars_, w))
        tight = np.full_like(vars_, 1e-4)
        out.append(("variance 1e-4 S%d M%d D%d" % (S, M, D), means[0, 0] + rng.normal(size=(N, D)) * 0.05, means, tight, w))
        wz = w.copy()
        wz[:, 0] = 0.0
        wz[0, :] = 0.0
        wz[1:] /= wz[1:].sum(axis=1, keepdims=True)
        out.append(("zero weights S%d M%d D%d" % (S, M, D), X, means, vars_, wz))
        # NaN constants: a negative variance in every component of state 0 (NaN, or +inf when the mixture is padded), in
        # one component of state 1 (NaN), and in all but a zero-weight component of the last state (+inf)
        if S < 3:
            continue
        vn, wn = vars_.copy(), w.copy()
        vn[0, :, 0] = -1.0
        vn[1, 0, 0] = -1.0
        vn[S - 1, 1:, 0] = -1.0
        wn[S - 1, 0] = 0.0
        out.append(("nan constants S%d M%d D%d" % (S, M, D), X, means, vn, wn))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=20000, help="frames of the bench workload to model (0: all)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    wl = bench.synth_workload(1002, 200)
    S = wl["W"] * wl["n"]
    means, vars_, w = wl["means"].reshape(S, wl["M"], wl["D"]), wl["vars"].reshape(S, wl["M"], wl["D"]), wl["w"].reshape(S, wl["M"])
    X = wl["X"] if not a.frames else wl["X"][:a.frames]
    cases = [("bench.synth_workload(1002, 200), %d frames" % len(X), X, means, vars_, w)] + edge_models()
    bad = 0
    for name, X, means, vars_, w in cases:
        for compat in (True, False):
            worst, wrong_inf = 0.0, 0
            cold_cells = cold_blocks = n_chunks = 0
            gap = []
            for i in range(0, len(X), 512):          # (chunks of whole 32-frame blocks: the [N,S,M,D] temporaries stay small)
                res = evaluate(X[i:i + 512], means, vars_, w, compat)
                e, wi, cc, cb = check(res, compat)
                worst, wrong_inf = max(worst, e), wrong_inf + wi
                cold_cells += cc * len(res["s"]); cold_blocks += cb * len(res["s"]); n_chunks += len(res["s"])
                gap.append((res["mh"][None] - res["amax"])[np.isfinite(res["amax"])])
            gap = np.concatenate([g.ravel() for g in gap]).astype(np.float64)
            print("%-44s compat=%d  max rel err %.2e  wrong +inf / NaN %d  redo: %.4f of cells, %.4f of 32-frame blocks  "
                  "mh - max a: %.1f .. %.1f nats" % (name, compat, worst, wrong_inf, cold_cells / n_chunks, cold_blocks / n_chunks,
                                                     gap.min() if len(gap) else 0, gap.max() if len(gap) else 0))
            bad += (worst > 1e-12) + (wrong_inf > 0)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
