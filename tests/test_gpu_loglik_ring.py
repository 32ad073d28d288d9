# -*- coding: utf-8 -*-
"""The operand ring of the matrix-core likelihood kernel (csrc/gh_loglik_mfma.hip): every slot is refilled
behind the MFMA pair that consumed it and waited for on a count, the refills of a tile's last k-steps fetch the NEXT
tile (the zero pad after the model's last one; tile `t_lo` of the next block in a wave that walks several blocks).  A
wrong slot, a wrong wait or a wrong wrap-around shows as a wrong likelihood, so every case is compared with the fp64
oracle and, bit for bit, across the launch forms that reach the same numbers through different rings:

* N = 70 frames: two full 32-frame blocks and a partial one;
* D = 3 and D = 39: 2 and 20 k-steps (a ring of 2 / 20 slots in fp64, 1 / 10 in fp32);
* fp64 and fp32;
* M = 1, 2, 8, 32: the epilogues beside the ring (M = 32: two tiles per state);
* S such that the model has 1, 2, 3 and 4 Gaussian tiles: the single tile whose "next tile" is the zero pad, both peeled
  tails of the two-tiles-per-iteration fp64 loop (M = 32 has an even number of tiles: 2 and 4);
* one block per wave (GMMHMM_LOGLIK_BPW=1), 2 and 4 blocks per wave (the closed loop over the tiles) and the host's own
  choice;
* the block-table launch (state_ranges) with a first tile other than 0 and a different tile range in the next block.

Tolerances: fp64 at 1e-10 relative against `oracle.ref_numpy`, the suite's bound for this kernel (tests/test_gpu_kernels.py);
fp32 at the suite's fp32 bound, 1e-3 (24-bit operands: 1e-10 is not representable there).  The launch forms must agree
exactly in both precisions: the change of the ring touches no arithmetic."""
import numpy as np
import pytest

from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

N = 70
TILE_ROWS = 16
# states for 1, 2, 3, 4 Gaussian tiles (n_tiles = ceil(S * M_pad / 16); M = 32: 2 tiles per state)
STATES = {1: [13, 29, 48, 61], 2: [7, 16, 21, 32], 8: [2, 3, 6, 7], 32: [1, 2]}
TILES = {1: [1, 2, 3, 4], 2: [1, 2, 3, 4], 8: [1, 2, 3, 4], 32: [2, 4]}


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def loglik(hip, ctx, gmm, X, offsets, dtype, **kw):
    b = hip.Batch(ctx, feats=X, offsets=offsets, dtype=dtype)
    try:
        return b.loglik(gmm, **kw).copy()
    finally:
        b.close()


@pytest.mark.parametrize("M", [1, 2, 8, 32])
@pytest.mark.parametrize("D", [3, 39])
@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-10), (np.float32, 1e-3)])
def test_ring_order_against_oracle_and_across_launch_forms(hip, ctx, monkeypatch, dtype, rtol, D, M):
    rng = np.random.default_rng(1000 * D + 10 * M + (dtype == np.float32))
    X = rng.normal(size=(N, D)) * 1.3
    for S, n_tiles in zip(STATES[M], TILES[M]):
        means = rng.normal(size=(S, M, D))
        vars_ = rng.uniform(0.5, 1.5, size=(S, M, D))
        w = rng.dirichlet(np.ones(M), size=S)
        ref = O.gmm_neg_loglik_batch(X, means, vars_, w)
        gmm = hip.PackedGMM(ctx, means, vars_, w)
        try:
            assert -(-S * M // TILE_ROWS) == n_tiles         # (M = 1, 2, 8, 32 are their own padded sizes)
            got = {}
            for bpw in (None, "1", "2", "4"):
                if bpw is None:
                    monkeypatch.delenv("GMMHMM_LOGLIK_BPW", raising=False)
                else:
                    monkeypatch.setenv("GMMHMM_LOGLIK_BPW", bpw)
                got[bpw] = loglik(hip, ctx, gmm, X, [0, N], dtype)
                assert got[bpw].shape == (N, S)
                np.testing.assert_allclose(got[bpw], ref, rtol=rtol, err_msg="S=%d (%d tiles) bpw=%s" % (S, n_tiles, bpw))
            for bpw in ("1", "2", "4"):
                np.testing.assert_array_equal(got[bpw], got[None], err_msg="S=%d (%d tiles) bpw=%s against the default" % (S, n_tiles, bpw))
            if n_tiles < 2 or (M > 16 and S < 2):            # (a single state of 32 components owns both of its tiles)
                continue
            # block table: utterance 0 = frames [0, 33) on the tiles [1, n_tiles), utterance 1 = frames [33, 70) on
            # tile 0 (M = 32: the tiles of state 0) -- a first tile other than 0, and a wrap to ANOTHER tile range when
            # a wave moves from the last block of utterance 0 to the first block of utterance 1
            per_tile = max(1, TILE_ROWS // M)            # states per tile (M = 32: a state is two tiles)
            first = per_tile if M <= 16 else 1           # first state of tile 1 (M = 32: of tile 2)
            lo, hi = [first, 0], [S, first]
            for bpw in (None, "2", "4"):
                if bpw is None:
                    monkeypatch.delenv("GMMHMM_LOGLIK_BPW", raising=False)
                else:
                    monkeypatch.setenv("GMMHMM_LOGLIK_BPW", bpw)
                sub = loglik(hip, ctx, gmm, X, [0, 33, N], dtype, state_ranges=(lo, hi))
                np.testing.assert_array_equal(sub[:33, first:], got[None][:33, first:], err_msg="subset S=%d bpw=%s, tiles from 1" % (S, bpw))
                np.testing.assert_array_equal(sub[33:, :first], got[None][33:, :first], err_msg="subset S=%d bpw=%s, tile 0" % (S, bpw))
                np.testing.assert_allclose(sub[:33, first:], ref[:33, first:], rtol=rtol)
                np.testing.assert_allclose(sub[33:, :first], ref[33:, :first], rtol=rtol)
        finally:
            monkeypatch.delenv("GMMHMM_LOGLIK_BPW", raising=False)
            gmm.close()
