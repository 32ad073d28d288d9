# -*- coding: utf-8 -*-
"""The fp64 likelihood kernel's log-sum-exp against the pack-time bound (csrc/gh_loglik_mfma.hip, BND): the
default fp64 epilogue of the one-tile-per-state mixture branches (M_pad = 2, 4, 8, 16), its guard and the redo in the
max-shifted form, and GMMHMM_LSE_BOUND=0, which launches the max-shifted form from the same library.

1. random models against the fp64 oracle (`O.gmm_neg_loglik_batch`) at 1e-11 relative, and the two forms against each
   other at 1e-12 relative (the largest difference seen is printed: DESIGN section 6 records it);
2. the redo: frames moved away from every mean until a state's log-sum-exp lies above the guard (2^-900 of the bound:
   -624 nats), between the guard and the reference's underflow limit (-745 nats), and beyond it -- finite values at 1e-11
   of the oracle on both sides of the guard, +inf exactly where the max-shifted form gives it; log domain throughout
   with set_compat(underflow=False); a block in which ONE frame needs the redo leaves the other rows bit for bit what
   they are without it;
3. variances of 1e-4 (the bound far above 0), zero-weight components, a state with every weight zero (+inf), a NaN
   feature (its own row only), NaN constants (negative variances) in one, in every, and in every switched-on component
   of a state: NaN / +inf where the max-shifted form has them;
4. the bitwise equalities the repository relies on: block table against full launch, one block per wave against
   several, a frame's position in its block.

Mixtures of more than 16 components (several tiles per state) keep the max-shifted form and are not covered here.

The shapes are the smallest that reach each branch; one oracle call per model."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

NS = [1, 17, 33, 69]
MS = [2, 4, 8, 16]                # M_pad = 2, 4, 8, 16: every branch of the bound epilogue
SS = [2, 50, 51, 70]              # exact cover / a partial last tile / more than 64 states: a second LDS chunk and table
LN2 = float(np.log(2.0))
GUARD = -900.0 * LN2              # ln 2^-900: the sum against the bound below which the tile is redone
COMPAT = -1075.0 * LN2            # the reference's linear-domain underflow limit


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@pytest.fixture(scope="module")
def ctx_log(hip):
    c = hip.Context(0)
    c.set_compat(underflow=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model_tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lse_bound_model.py")
    spec = importlib.util.spec_from_file_location("lse_bound_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_model(rng, S, M, D):
    return (rng.normal(size=(S, M, D)), rng.uniform(0.5, 1.5, size=(S, M, D)), rng.dirichlet(np.ones(M), size=S))


def loglik(hip, ctx, gmm, X, offsets, **kw):
    b = hip.Batch(ctx, feats=X, offsets=offsets, dtype=np.float64)
    try:
        return b.loglik(gmm, **kw).copy()
    finally:
        b.close()


def set_bpw(monkeypatch, bpw):
    if bpw is None:
        monkeypatch.delenv("GMMHMM_LOGLIK_BPW", raising=False)
    else:
        monkeypatch.setenv("GMMHMM_LOGLIK_BPW", bpw)


def max_rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.abs(a - b) / np.abs(b)))


# ------------------------------------------------------------------------------------------ 1 and 5
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", [3, 39])
def test_random_models_against_oracle_and_max_shifted_form(hip, ctx, monkeypatch, D, M):
    rng = np.random.default_rng(300 * D + M)
    X = rng.normal(size=(max(NS), D)) * 1.3
    worst_forms = 0.0
    for S in SS:
        means, vars_, w = random_model(rng, S, M, D)
        ref = O.gmm_neg_loglik_batch(X, means, vars_, w)
        gmm = hip.PackedGMM(ctx, means, vars_, w)
        try:
            for bpw in (None, "1", "3"):
                set_bpw(monkeypatch, bpw)
                for N in NS:
                    monkeypatch.delenv("GMMHMM_LSE_BOUND", raising=False)
                    got = loglik(hip, ctx, gmm, X[:N], [0, N])
                    assert got.shape == (N, S)
                    np.testing.assert_allclose(got, ref[:N], rtol=1e-11, err_msg="S=%d N=%d bpw=%s" % (S, N, bpw))
                    monkeypatch.setenv("GMMHMM_LSE_BOUND", "0")
                    old = loglik(hip, ctx, gmm, X[:N], [0, N])
                    monkeypatch.delenv("GMMHMM_LSE_BOUND", raising=False)
                    np.testing.assert_allclose(old, ref[:N], rtol=1e-11, err_msg="max-shifted form S=%d N=%d bpw=%s" % (S, N, bpw))
                    worst_forms = max(worst_forms, max_rel(got, old))
                    np.testing.assert_allclose(got, old, rtol=1e-12, atol=0, err_msg="forms S=%d N=%d bpw=%s" % (S, N, bpw))
        finally:
            gmm.close()
    print("D=%d M=%d: largest relative difference between the bound form and the max-shifted form %.3e" % (D, M, worst_forms))


# ------------------------------------------------------------------------------------------ 2: the redo
def far_frames(rng, means, n_frames, lo=-420.0, hi=-1100.0):
    """Frames on a ray from the centre of the means, at distances that put -r^2/2 between lo and hi nats"""
    D = means.shape[-1]
    centre = means.reshape(-1, D).mean(axis=0)
    u = rng.normal(size=D)
    u /= np.linalg.norm(u)
    r = np.sqrt(-2.0 * np.linspace(lo, hi, n_frames))
    return centre[None] + r[:, None] * u[None]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", [3, 39])
def test_redo_on_both_sides_of_the_guard_and_of_the_underflow_limit(hip, ctx, ctx_log, monkeypatch, model_tool, D, M):
    rng = np.random.default_rng(700 * D + M)
    S = 5
    means, vars_, w = random_model(rng, S, M, D)
    vars_ = rng.uniform(0.9, 1.1, size=vars_.shape)
    X = far_frames(rng, means, 69)
    ref = O.gmm_neg_loglik_batch(X, means, vars_, w)
    C, mh, _ = model_tool.pack(means, vars_, w)
    level = -ref - np.asarray(mh, dtype=np.float64)[None]         # the state's log-sum-exp against its bound, nats
    above, between, beyond = level > GUARD + 5, (level < GUARD - 5) & (-ref > COMPAT + 5), -ref < COMPAT - 5
    assert above.any() and between.any() and beyond.any(), "the frames do not reach every regime"
    for bpw in (None, "1", "3"):
        set_bpw(monkeypatch, bpw)
        gmm = hip.PackedGMM(ctx, means, vars_, w)
        try:
            got = loglik(hip, ctx, gmm, X, [0, 69])
            monkeypatch.setenv("GMMHMM_LSE_BOUND", "0")
            old = loglik(hip, ctx, gmm, X, [0, 69])
            monkeypatch.delenv("GMMHMM_LSE_BOUND", raising=False)
        finally:
            gmm.close()
        # (a) compat mode: +inf exactly where the max-shifted form gives it, the oracle's value everywhere else
        np.testing.assert_array_equal(np.isinf(got), np.isinf(old))
        assert np.isinf(got[beyond]).all() and np.isfinite(got[above | between]).all()
        fin = np.isfinite(got)
        print("D=%d M=%d bpw=%s compat: above the guard %.2e, redone %.2e (max rel. error against the oracle)"
              % (D, M, bpw, max_rel(got[above], ref[above]), max_rel(got[between], ref[between])))
        np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-11)
        # (b) log domain throughout: thousands of nats out, finite, the oracle's value
        far = np.concatenate([X, far_frames(rng, means, 17, -3000.0, -60000.0)])
        ref_far = O.gmm_neg_loglik_batch(far[69:], means, vars_, w)
        gmm = hip.PackedGMM(ctx_log, means, vars_, w)
        try:
            got_log = loglik(hip, ctx_log, gmm, far, [0, len(far)])
        finally:
            gmm.close()
        assert np.isfinite(got_log).all()
        np.testing.assert_allclose(got_log[:69], ref, rtol=1e-11)
        np.testing.assert_allclose(got_log[69:], ref_far, rtol=1e-11)


@pytest.mark.parametrize("M", MS)
def test_one_redone_frame_leaves_its_block_alone(hip, ctx, monkeypatch, M):
    """Row 13 of a 32-frame block is moved 800 nats out: the tile's epilogue is redone for the wave, the other 31 rows are
    bit for bit what they are in a batch where no row needs it."""
    rng = np.random.default_rng(40 + M)
    S, D = 7, 39
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(32, D)) * 1.3
    bad = X.copy()
    bad[13] = far_frames(rng, means, 1, -800.0, -800.0)[0]
    keep = np.arange(32) != 13
    gmm = hip.PackedGMM(ctx, means, vars_, w)
    try:
        clean = loglik(hip, ctx, gmm, X, [0, 32])
        got = loglik(hip, ctx, gmm, bad, [0, 32])
        monkeypatch.setenv("GMMHMM_LSE_BOUND", "0")
        old = loglik(hip, ctx, gmm, bad, [0, 32])
        monkeypatch.delenv("GMMHMM_LSE_BOUND", raising=False)
    finally:
        gmm.close()
    ref = O.gmm_neg_loglik_batch(bad, means, vars_, w)
    np.testing.assert_array_equal(got[keep], clean[keep])
    np.testing.assert_array_equal(np.isinf(got), np.isinf(old))
    assert np.isinf(got[13]).any()
    fin = np.isfinite(got)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-11)


# ------------------------------------------------------------------------------------------ 3: corners of the packing
@pytest.mark.parametrize("M", MS)
def test_tight_variances_zero_weights_and_a_switched_off_state(hip, ctx_log, ctx, monkeypatch, M):
    rng = np.random.default_rng(90 + M)
    S, D = 51, 3
    means = rng.normal(size=(S, M, D))
    vars_ = np.full((S, M, D), 1e-4)                                # C_g = log w + 11.1 nats: the bound is far above 0
    w = rng.dirichlet(np.ones(M), size=S)
    w[:, 0] = 0.0                                                   # a zero-weight component in every state
    w[3, :] = 0.0                                                   # a state with no component at all
    w[np.arange(S) != 3] /= w[np.arange(S) != 3].sum(axis=1, keepdims=True)
    X = means[rng.integers(0, S, size=33), 1] + 0.01 * rng.normal(size=(33, D))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = O.gmm_neg_loglik_batch(X, means, vars_, w)
    on = np.arange(S) != 3
    for c in (ctx_log, ctx):
        gmm = hip.PackedGMM(c, means, vars_, w)
        try:
            got = loglik(hip, c, gmm, X, [0, 33])
            monkeypatch.setenv("GMMHMM_LSE_BOUND", "0")
            old = loglik(hip, c, gmm, X, [0, 33])
            monkeypatch.delenv("GMMHMM_LSE_BOUND", raising=False)
        finally:
            gmm.close()
        assert np.isposinf(got[:, 3]).all()
        np.testing.assert_array_equal(np.isinf(got), np.isinf(old))
        if c is ctx_log:
            np.testing.assert_allclose(got[:, on], ref[:, on], rtol=1e-11)
        else:       # linear-domain underflow of the reference: +inf where every weighted density is below 2^-1075
            fin = np.isfinite(got[:, on])
            np.testing.assert_allclose(got[:, on][fin], ref[:, on][fin], rtol=1e-11)
            assert fin.any()


@pytest.mark.parametrize("M", MS)
def test_nan_feature_poisons_its_own_row_only(hip, ctx, M):
    rng = np.random.default_rng(60 + M)
    S, D = 50, 39
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(69, D)) * 1.3
    bad = X.copy()
    bad[3, 0] = bad[17, D - 1] = bad[68, D // 2] = np.nan
    rows = np.zeros(69, dtype=bool)
    rows[[3, 17, 68]] = True
    gmm = hip.PackedGMM(ctx, means, vars_, w)
    try:
        clean = loglik(hip, ctx, gmm, X, [0, 69])
        got = loglik(hip, ctx, gmm, bad, [0, 69])
    finally:
        gmm.close()
    assert np.isfinite(clean).all() and np.isnan(got[rows]).all()
    np.testing.assert_array_equal(got[~rows], clean[~rows])


# ------------------------------------------------------------------------------------------ 4: bitwise equalities
@pytest.mark.parametrize("S,M,D", [(50, 8, 39), (51, 2, 3), (51, 4, 3), (70, 16, 39)])
def test_block_table_bpw_and_position_bitwise(hip, ctx, monkeypatch, S, M, D):
    rng = np.random.default_rng(S + 3 * M + D)
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(69, D)) * 1.3
    X[40] = far_frames(rng, means, 1, -800.0, -800.0)[0]            # (one frame on the redo: the equalities hold there too)
    off = [0, 1, 69]
    r_off, r_lo, r_hi = [0, 1, 3], [0, 0, S - 4], [3, 2, S]
    gmm = hip.PackedGMM(ctx, means, vars_, w)
    try:
        monkeypatch.delenv("GMMHMM_LOGLIK_BPW", raising=False)
        full = loglik(hip, ctx, gmm, X, off)
        sets = loglik(hip, ctx, gmm, X, off, state_sets=(r_off, r_lo, r_hi))
        for u in range(2):
            rows = slice(off[u], off[u + 1])
            for r in range(r_off[u], r_off[u + 1]):
                np.testing.assert_array_equal(sets[rows, r_lo[r]:r_hi[r]], full[rows, r_lo[r]:r_hi[r]])
        by_bpw = {}
        for bpw in ("1", "3"):
            monkeypatch.setenv("GMMHMM_LOGLIK_BPW", bpw)
            by_bpw[bpw] = loglik(hip, ctx, gmm, X, off)
        np.testing.assert_array_equal(by_bpw["1"], by_bpw["3"])
        np.testing.assert_array_equal(by_bpw["1"], full)
        monkeypatch.delenv("GMMHMM_LOGLIK_BPW", raising=False)
        for k in (1, 7, 16, 31):
            np.testing.assert_array_equal(loglik(hip, ctx, gmm, X[k:], [0, 69 - k]), full[k:])
    finally:
        gmm.close()


@pytest.mark.parametrize("M", [2, 3, 4, 8, 16])
def test_nan_constants_as_in_the_max_shifted_form(hip, ctx, ctx_log, monkeypatch, M):
    """A negative variance makes a component's constant NaN.  State 0: in every component (NaN when the padded mixture
    has no other slot, +inf when mixture padding supplies a switched-off one: M = 3); state 1: in one component (NaN);
    state 2: in every component but a zero-weight one (+inf); the states beside them are untouched."""
    rng = np.random.default_rng(20 + M)
    S, D = 7, 3
    means, vars_, w = random_model(rng, S, M, D)
    vars_[0, :, 0] = -1.0
    vars_[1, 0, 0] = -1.0
    vars_[2, 1:, 0] = -1.0
    w[2, 0] = 0.0
    X = rng.normal(size=(33, D)) * 1.3
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = O.gmm_neg_loglik_batch(X, means, vars_, w)
    for c in (ctx, ctx_log):
        gmm = hip.PackedGMM(c, means, vars_, w)
        try:
            got = loglik(hip, c, gmm, X, [0, 33])
            monkeypatch.setenv("GMMHMM_LSE_BOUND", "0")
            old = loglik(hip, c, gmm, X, [0, 33])
            monkeypatch.delenv("GMMHMM_LSE_BOUND", raising=False)
        finally:
            gmm.close()
        np.testing.assert_array_equal(np.isnan(got), np.isnan(old))
        np.testing.assert_array_equal(np.isinf(got), np.isinf(old))
        assert np.isnan(got[:, 1]).all() and np.isposinf(got[:, 2]).all()
        assert (np.isnan(got[:, 0]) if M in (2, 4, 8, 16) else np.isposinf(got[:, 0])).all()
        np.testing.assert_allclose(got[:, 3:], ref[:, 3:], rtol=1e-11)
