# -*- coding: utf-8 -*-
"""The matrix-core likelihood kernel (csrc/gh_loglik_mfma.hip) at the edges of its frame blocks and of its state tiles: the
frame operands are guarded by the block's row count and by D, and only the epilogue of a block's last tile tests the
state index against S (the tile loop stores without the test).

* against the fp64 oracle (`O.gmm_neg_loglik_batch`) at the tolerances of test_gpu_kernels.test_loglik_vs_oracle_shapes
  (1e-11 relative in fp64, 1e-3 in fp32), over frame counts around the 16-frame column tile and the 32-frame block,
  every padded operand length, every mixture branch of the epilogue, state counts that fill their tiles exactly, leave a
  partial last tile, or need more than one LDS chunk -- with one and with several blocks per wave;
* a block-table launch over utterances of 1 and 33 frames with two state ranges over the same frames;
* position independence, bitwise: a frame's column of the GEMM never mixes with its neighbours, so its likelihoods do
  not depend on where in a block it sits (the online-vs-offline tests rely on it);
* a NaN feature poisons its own row only.

One oracle call per (D, M, S) on 69 frames; the shorter batches are prefixes of it (the oracle works row by row)."""
import numpy as np
import pytest

from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

NS = [1, 15, 16, 17, 31, 32, 33, 69]
DS = [3, 13, 24, 39, 41]          # KP = 4, 16, 24 (no padding), 40, 48
MS = [1, 2, 4, 8, 16, 20]         # M_pad = 1, 2, 4, 8, 16, 32: every branch of the tile epilogue
SS = [1, 2, 50, 51, 70]           # exact cover / a partial last tile / more than 64 states: a chunked flush
TOL = {np.float64: 1e-11, np.float32: 1e-3}


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def random_model(rng, S, M, D):
    return (rng.normal(size=(S, M, D)), rng.uniform(0.5, 1.5, size=(S, M, D)), rng.dirichlet(np.ones(M), size=S))


def loglik(hip, ctx, gmm, X, offsets, dtype, **kw):
    b = hip.Batch(ctx, feats=X, offsets=offsets, dtype=dtype)
    try:
        return b.loglik(gmm, **kw).copy()
    finally:
        b.close()


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", DS)
def test_against_oracle(hip, ctx, monkeypatch, D, M):
    rng = np.random.default_rng(100 * D + M)
    X = rng.normal(size=(max(NS), D)) * 1.3
    for S in SS:
        means, vars_, w = random_model(rng, S, M, D)
        ref = O.gmm_neg_loglik_batch(X, means, vars_, w)
        gmm = hip.PackedGMM(ctx, means, vars_, w)
        try:
            for bpw in (None, "1", "3"):      # the launcher's choice, one block per wave, several blocks per wave
                if bpw is None:
                    monkeypatch.delenv("GMMHMM_LOGLIK_BPW", raising=False)
                else:
                    monkeypatch.setenv("GMMHMM_LOGLIK_BPW", bpw)
                for dtype, rtol in TOL.items():
                    for N in NS:
                        got = loglik(hip, ctx, gmm, X[:N], [0, N], dtype)
                        assert got.shape == (N, S)
                        np.testing.assert_allclose(got, ref[:N], rtol=rtol, err_msg="S=%d N=%d bpw=%s %s" % (S, N, bpw, dtype.__name__))
        finally:
            gmm.close()


@pytest.mark.parametrize("S,M,D", [(50, 8, 39), (51, 2, 13), (70, 20, 41), (12, 1, 3)])
def test_block_table_two_ranges_over_the_same_frames(hip, ctx, S, M, D):
    """Utterances of 1 and 33 frames; the second has two state ranges that do not touch, so the table holds two entries
    for each of its frame blocks and the wave builds their operands once."""
    rng = np.random.default_rng(S + M + D)
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(34, D)) * 1.3
    off = [0, 1, 34]
    ref = O.gmm_neg_loglik_batch(X, means, vars_, w)
    hi0 = min(S, 3)
    r_off, r_lo, r_hi = [0, 1, 3], [0, 0, S - min(S, 4)], [hi0, min(S, 2), S]
    if r_hi[1] >= r_lo[2]:      # (S too small for two separate ranges: the same range twice)
        r_lo[2], r_hi[2] = r_lo[1], r_hi[1]
    gmm = hip.PackedGMM(ctx, means, vars_, w)
    try:
        for dtype, rtol in TOL.items():
            full = loglik(hip, ctx, gmm, X, off, dtype)
            sets = loglik(hip, ctx, gmm, X, off, dtype, state_sets=(r_off, r_lo, r_hi))
            rng_ = loglik(hip, ctx, gmm, X, off, dtype, state_ranges=(np.array([0, r_lo[2]], dtype=np.int32),
                                                                        np.array([hi0, r_hi[2]], dtype=np.int32)))
            for u in range(2):
                rows = slice(off[u], off[u + 1])
                for r in range(r_off[u], r_off[u + 1]):
                    cols = slice(r_lo[r], r_hi[r])
                    np.testing.assert_array_equal(sets[rows, cols], full[rows, cols])
                    np.testing.assert_allclose(sets[rows, cols], ref[rows, cols], rtol=rtol)
            np.testing.assert_array_equal(rng_[0:1, 0:hi0], full[0:1, 0:hi0])
            np.testing.assert_array_equal(rng_[1:34, r_lo[2]:r_hi[2]], full[1:34, r_lo[2]:r_hi[2]])
    finally:
        gmm.close()


@pytest.mark.parametrize("S,M,D", [(50, 8, 39), (51, 1, 13), (70, 20, 41), (7, 4, 24)])
def test_position_independence_bitwise(hip, ctx, S, M, D):
    rng = np.random.default_rng(7 * S + M + D)
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(69, D)) * 1.3
    gmm = hip.PackedGMM(ctx, means, vars_, w)
    try:
        for dtype in TOL:
            whole = loglik(hip, ctx, gmm, X, [0, 69], dtype)
            for k in (1, 7, 16, 31):
                np.testing.assert_array_equal(loglik(hip, ctx, gmm, X[k:], [0, 69 - k], dtype), whole[k:])
    finally:
        gmm.close()


@pytest.mark.parametrize("S,M,D", [(50, 8, 39), (51, 1, 13), (70, 20, 41), (7, 4, 24)])
def test_nan_feature_stays_in_its_row(hip, ctx, S, M, D):
    """NaN in the first dimension, in the last one (the neighbour in memory of the next frame's first) and in the last
    frame of the batch: those rows are NaN, every other row is bit for bit what it is without them."""
    rng = np.random.default_rng(11 * S + M + D)
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(69, D)) * 1.3
    bad = X.copy()
    bad[3, 0] = bad[17, D - 1] = bad[31, D // 2] = bad[68, D - 1] = np.nan
    rows = np.zeros(69, dtype=bool)
    rows[[3, 17, 31, 68]] = True
    gmm = hip.PackedGMM(ctx, means, vars_, w)
    try:
        for dtype in TOL:
            clean = loglik(hip, ctx, gmm, X, [0, 69], dtype)
            got = loglik(hip, ctx, gmm, bad, [0, 69], dtype)
            assert np.isfinite(clean).all()
            assert np.isnan(got[rows]).all()
            np.testing.assert_array_equal(got[~rows], clean[~rows])
    finally:
        gmm.close()
