# -*- coding: utf-8 -*-
"""Online decoding with a bigram grammar of 17 to 64 words on the device (gh_viterbi_bigram_online_wide.hip,
gh_online_create_bigram_wide): the WIDE BIGRAM sweep carried across chunks, one wave per stream, four streams per block
around one LDS image of the word-to-word costs.

The contract is "online == offline on the prefix", held against the one-shot wide bigram kernel ON THE SAME LIKELIHOODS
with assert_array_equal: end costs, chosen ends, paths, labels, begins.
  1. every N x skip instantiation in both dtypes, word counts 17 / 33 / 49 / 64 rotating, random column ranges;
  2. chunk lengths 1, 2, 3, 4, 5, 7 and 9 in one run, and strictly one frame per push;
  3. blocks of four waves with one to three idle waves, and counts of 1 and 40 in one block;
  4. predecessor ties between words of different 16-lane groups, one frame at a time;
  5. an entry row whose candidates are all +inf, carried over three pushes;
  6. a reused id after reset against a fresh session, and column 0 of a one-frame stream;
  7. running results at every 20-frame tick against decode_batch of the prefix;
  8. audio through a StreamingFrontend;
  9. refusals through the real library."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bigram_wide import (all_inf_entry_case, check_against_oracle, dense_of, make_model, packed, random_costs,
                                  word_trans)
from test_gpu_online_wide import make_hmm, make_utts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import sr.recognition as R
    return R


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def make_decoder(R, ctx, rng, W, n, skip, forbid=0.2, M=2, D=6, dtype=np.float64):
    """A bigram decoder of W toy words with random word-to-word costs, a fraction `forbid` of them +inf."""
    from sr.recognition.batch import ContinuousDecoder
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    hmms = [make_hmm(R, means[i], vars_[i], w[i], word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3))) for i in range(W)]
    B, init = random_costs(rng, W, forbid)
    dec = ContinuousDecoder(hmms, grammar="bigram", bigram=B, initial=init, dtype=dtype, ctx=ctx)
    assert "bigram_wide" in dec.lat.forms() and "bigram" not in dec.lat.forms()
    return dec, means, vars_


def assert_bitwise_the_one_shot_decode(dec, on, ids, b, n):
    """`on` (times=True) has taken the whole batch `b` on the streams `ids`: everything equals the one-shot wide bigram
    kernel on the same likelihood matrix."""
    row_word = np.where(dec.row_state >= 0, dec.row_state // n, -1).astype(np.int32)
    np.testing.assert_array_equal(on.frames[ids], np.asarray(b.lengths, dtype=np.int64))
    ref = dec.lat.viterbi(b, want_path=True)
    words, info = on.result(ids, want_path=True)
    np.testing.assert_array_equal(info["end_cost"].reshape(-1), ref["end_cost_flat"])
    np.testing.assert_array_equal(info["best_end"], ref["best_end"])
    assert np.isfinite(ref["end_cost_flat"]).any()
    for u in range(b.U):
        np.testing.assert_array_equal(info["paths"][u], ref["paths"][u])
    lab = dec.lat.viterbi_labels(b, row_word, max_labels=dec._max_labels(b.lengths), want_begin=True)
    words2, info2 = on.result(ids)
    assert words2 == [[int(v) for v in l] for l in lab["labels"]] == words
    for u in range(b.U):
        np.testing.assert_array_equal(info2["begins"][u], lab["begins"][u])   # the timed label mode of the wide back-trace
        np.testing.assert_array_equal(info["begins"][u], lab["begins"][u])    # (the host rule on the path)
    np.testing.assert_array_equal(info2["end_cost"].reshape(-1), ref["end_cost_flat"])
    np.testing.assert_array_equal(info2["best_end"], ref["best_end"])
    return words


# ----------------------------------------------------------------------------------------------------------------------
# 1. every instantiation: the 13 N x skip shapes, the word counts one past each 16-lane group boundary and the full wave
SHAPES = [(n, s) for n in range(2, 9) for s in (False, True) if n > 2 or not s]
WORDS = (17, 33, 49, 64)


@pytest.mark.parametrize("k,n,skip", [(k, n, s) for k, (n, s) in enumerate(SHAPES)])
def test_online_bigram_wide_sweep_is_bitwise_the_one_shot_kernel(R, hip, ctx, k, n, skip):
    """One whole-utterance batch with resident likelihoods, fed through push_batch(first, count) in random column ranges (0-
    and 1-frame ranges among them); 13 ragged utterances, some shorter than a word, on ids scattered over 19 streams (five
    blocks, the last with one idle wave or more); 20 % forbidden word pairs; both dtypes."""
    W = WORDS[k % 4]
    rng = np.random.default_rng(91 * W + 7 * n + skip)
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, skip)
    xs = make_utts(rng, means, vars_, 13, words=(1, 5))
    for dtype in (np.float64, np.float32):
        b = hip.Batch(ctx, xs, dtype=dtype)
        T = np.asarray(b.lengths, dtype=np.int64)
        on = dec.online_bigram(n_streams=19, max_frames=int(T.max()), times=True, wide=True)
        assert isinstance(on.session, hip.OnlineBigramWideSession) and not on.settles
        ids = rng.permutation(19)[:b.U]
        pos = np.zeros(b.U, dtype=np.int64)
        while np.any(pos < T):
            cnt = np.minimum(rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 1000], size=b.U), T - pos)
            on.push_batch(ids, b, first=pos, count=cnt)                 # (the first call computes the likelihoods, once)
            pos += cnt
        words = assert_bitwise_the_one_shot_decode(dec, on, ids, b, n)
        assert any(len(wd) >= 2 for wd in words)
        on.close()
        b.close()


# ----------------------------------------------------------------------------------------------------------------------
# 2. chunk lengths
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_bigram_wide_chunk_lengths_and_one_frame_at_a_time(R, hip, ctx, dtype):
    """Chunks of 1, 2, 3, 4, 5, 7 and 9 frames in one run, every stream starting elsewhere in that cycle: the PF = 4 group
    loop with every tail length and the clamped refill.  Then the same utterances strictly ONE frame per push: the start-row
    term of column 0 and the history address of every single column."""
    W, n = 33, 5
    rng = np.random.default_rng(3305)
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, True)
    xs = [x[:60] for x in make_utts(rng, means, vars_, 10, short_every=0, words=(4, 7))]
    b = hip.Batch(ctx, xs, dtype=dtype)
    T = np.asarray(b.lengths, dtype=np.int64)
    assert T.min() >= 31                                                  # (a whole cycle of chunk lengths fits)
    cycle = np.array([1, 2, 3, 4, 5, 7, 9])
    on = dec.online_bigram(n_streams=10, max_frames=60, times=True, wide=True)
    ids = rng.permutation(10)
    pos = np.zeros(b.U, dtype=np.int64)
    full = set()
    step = 0
    while np.any(pos < T):
        want = cycle[(np.arange(b.U) + step) % len(cycle)]
        cnt = np.minimum(want, T - pos)
        full.update(int(c) for c, q in zip(cnt, want) if c == q)
        on.push_batch(ids, b, first=pos, count=cnt)
        pos += cnt
        step += 1
    assert full == set(cycle.tolist())
    assert_bitwise_the_one_shot_decode(dec, on, ids, b, n)
    on.reset()
    for t in range(int(T.max())):
        on.push_batch(ids, b, first=np.minimum(t, T), count=(t < T).astype(np.int64))
    assert_bitwise_the_one_shot_decode(dec, on, ids, b, n)
    on.close()
    b.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. partly filled blocks
def test_online_bigram_wide_partly_filled_blocks(R, hip, ctx):
    """Pushes to 1, 3, 5 and 9 streams (the others sit the call out and never reach the device): the last block of four
    waves has three, one, three and three idle waves behind the barrier.  The three-stream push gives counts of 40, 1 and 17
    to the waves of ONE block."""
    W, n = 49, 4
    rng = np.random.default_rng(4904)
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, False)
    xs = [x[:60] for x in make_utts(rng, means, vars_, 9, short_every=0, words=(6, 8))]
    b = hip.Batch(ctx, xs)
    T = np.asarray(b.lengths, dtype=np.int64)
    assert T.min() >= 45
    on = dec.online_bigram(n_streams=12, max_frames=60, times=True, wide=True)
    ids = rng.permutation(12)[:9]
    pos = np.zeros(9, dtype=np.int64)
    plan = [{4: 3},                                                       # one stream
            {0: 40, 4: 1, 7: 17},                                         # three streams, one block: 40, 17, 1
            {1: 2, 2: 9, 3: 6, 5: 1, 8: 4}]                               # five streams: a full block and one wave
    for counts in plan:
        cnt = np.zeros(9, dtype=np.int64)
        for u, c in counts.items():
            cnt[u] = c
        on.push_batch(ids, b, first=pos, count=cnt)
        pos += cnt
    assert np.all(pos < T) and np.all(pos[[0, 4, 7]] > 0)
    on.push_batch(ids, b, first=pos)                                      # nine streams: two full blocks and one wave
    assert_bitwise_the_one_shot_decode(dec, on, ids, b, n)
    on.close()
    b.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. ties
def test_online_bigram_wide_breaks_predecessor_ties_like_the_one_shot_kernel(hip, ctx):
    """Small-integer costs over word models that come in identical pairs 20 words apart (words k and k + 20 share their
    Gaussians and their rows of B): two predecessor words of DIFFERENT 16-lane groups reach an entry row at exactly the
    same cost, and the merge of the groups must keep the lower one, as the one-shot kernel and the reference (np.argmin's
    first minimum) do.  One frame per push.  From the oracle's own cost matrices: some entry-row cell ON a decoded path had
    equal minimal candidates in two groups."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(4344)
    W, n, M, D = 40, 3, 1, 4
    half = make_model(rng, W // 2, n, M, D)
    means, vars_, w = (np.tile(a, (2,) + (1,) * (a.ndim - 1)) for a in half)
    t1 = [word_trans(rng, n, integer=True) for _ in range(W // 2)]
    wt = [t1[i % (W // 2)] for i in range(W)]
    Bh = rng.integers(0, 4, size=(W // 2, W)).astype(np.float64)
    B = np.tile(Bh, (2, 1))                                               # rows k and k + 20 equal: the twins tie as predecessors
    init = np.tile(rng.integers(0, 3, size=W // 2), 2).astype(np.float64)
    xs = []
    for seq in ([20, 5, 38], [31, 17, 24], [9, 36], [26, 33, 3], [18, 22, 28], [4, 39, 12]):
        segs = []
        for wd in seq:
            Tw = int(rng.integers(n, 2 * n + 3))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            segs.append(means[wd, st, 0] + np.sqrt(vars_[wd, st, 0]) * rng.normal(size=(Tw, D)))
        xs.append(np.concatenate(segs))
    gmm = packed(hip, ctx, means, vars_, w)
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    lat = hip.Lattices(ctx, [graph])
    assert "bigram_wide" in lat.forms()
    b = hip.Batch(ctx, xs)
    nll = b.loglik(gmm)
    T = np.asarray(b.lengths, dtype=np.int64)
    s = hip.OnlineBigramWideSession(ctx, lat, b.U, int(T.max()))
    ids = np.arange(b.U, dtype=np.int64)
    for t in range(int(T.max())):
        s.push(b, ids, first=np.minimum(t, T), count=(t < T).astype(np.int64))
    ref = lat.viterbi(b, want_path=True)
    got = s.result(ids, want_path=True)
    np.testing.assert_array_equal(got["end_cost"].reshape(-1), ref["end_cost_flat"])
    np.testing.assert_array_equal(got["best_end"], ref["best_end"])
    for u in range(b.U):
        np.testing.assert_array_equal(got["paths"][u], ref["paths"][u])
    dense = dense_of(graph)
    first = 1 + W * (n - 1)
    ties_across = 0
    for costs, path in check_against_oracle(graph, got, nll, b.offsets, rtol=1e-10):
        for row, col in path:
            if first <= row < first + W:
                cand = dense[row] + costs[:, col]
                at = (np.flatnonzero(cand == cand.min()) - 1) // (n - 1)      # the tied predecessor words
                ties_across += int(len(at) > 1 and np.isfinite(cand.min()) and at[0] // 16 != at[-1] // 16)
    assert ties_across >= 1, ties_across
    s.close(); b.close(); lat.close(); gmm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. an entry row whose every candidate is +inf
def test_online_bigram_wide_entry_row_with_only_infinite_candidates(hip, ctx):
    """test_gpu_bigram_wide.all_inf_entry_case (word 7 is entered from words 40 and 50 only, whose last states are +inf in
    every column) carried over three pushes: the records say word 0, which has no arc into that row, and the one-shot
    back-trace on the history replaces it by word 40 from the arc mask.  With every word's end and with word 7's end
    alone: end costs, ends and paths equal the one-shot decode's."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    W, n, means, vars_, w, wt, B, init, xs = all_inf_entry_case(np.random.default_rng(66))
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    ends = np.asarray(graph["end_rows"])
    g7 = dict(graph, end_rows=np.array([ends[7]], dtype=np.int32))
    first = 1 + W * (n - 1)
    gmm = packed(hip, ctx, means, vars_, w)
    b = hip.Batch(ctx, xs)
    b.loglik(gmm, fetch=False)
    T = np.asarray(b.lengths, dtype=np.int64)
    ids = np.arange(b.U, dtype=np.int64)
    through = 0
    for g in (graph, g7):
        lat = hip.Lattices(ctx, [g])
        assert "bigram_wide" in lat.forms()
        s = hip.OnlineBigramWideSession(ctx, lat, b.U, int(T.max()))
        cuts = [np.zeros(b.U, dtype=np.int64), T // 3, 2 * T // 3 + 1, T]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            s.push(b, ids, first=lo, count=hi - lo)
        ref = lat.viterbi(b, want_path=True)
        got = s.result(ids, want_path=True)                               # (a tripped flag raises)
        np.testing.assert_array_equal(got["end_cost"].reshape(-1), ref["end_cost_flat"])
        np.testing.assert_array_equal(got["best_end"], ref["best_end"])
        for u in range(b.U):
            np.testing.assert_array_equal(got["paths"][u], ref["paths"][u])
        if g is g7:
            for path in got["paths"]:
                rows = [int(p[0]) for p in path]
                for k in range(len(rows) - 1):
                    if rows[k] == first + 7:
                        assert rows[k + 1] == 1 + 40 * (n - 1) + n - 2    # the last state of word 40
                        through += 1
        s.close()
        lat.close()
    assert through >= 4, "the paths do not stand on the all-inf entry row"
    b.close(); gmm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 6. reuse and column 0
def test_online_bigram_wide_reused_id_equals_a_fresh_session(R, hip, ctx):
    """Streams take half of ANOTHER utterance, are reset, and take their own, while one stream sits ticks out: what the
    first utterance left in the carried column and in the history must not show.  Bitwise a fresh session."""
    W, n = 40, 3
    rng = np.random.default_rng(940)
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, True, forbid=0.1)
    pool = sorted(make_utts(rng, means, vars_, 7, short_every=0, words=(2, 6)), key=len)
    decoys = hip.Batch(ctx, [pool[-1], pool[-2], pool[3]])
    own = hip.Batch(ctx, [pool[0], pool[1], pool[3]])                       # shorter than the decoys: old history lies behind
    cap = len(pool[-1])
    on = dec.online_bigram(n_streams=5, max_frames=cap, times=True, wide=True)
    half = [len(pool[-1]) // 2, len(pool[-2]) // 2]
    on.push_batch([4, 1, 2], decoys, first=[0, 0, 0], count=half + [3])
    assert on.frames.tolist() == [0, half[1], 3, 0, half[0]]
    on.reset([4, 1])
    assert on.frames.tolist() == [0, 0, 3, 0, 0] == on.session.frames().tolist()
    k = 2
    on.push_batch([4, 1, 2], own, first=[0, 0, 3], count=[k, len(pool[1]), 0])      # stream 2 sits this tick out
    on.push_batch([4, 1, 2], own, first=[k, len(pool[1]), 3], count=[len(pool[0]) - k, 0, len(pool[3]) - 3])
    fresh = dec.online_bigram(n_streams=5, max_frames=cap, times=True, wide=True)
    fresh.push_batch([0, 3, 2], decoys, count=[0, 0, 3])                  # (the same likelihood values as stream 2 above)
    fresh.push_batch([0, 3, 2], own, first=[0, 0, 3])
    for want_path in (False, True):
        got, gi = on.result([4, 1, 2], want_path=want_path)
        exp, ei = fresh.result([0, 3, 2], want_path=want_path)
        assert got == exp
        np.testing.assert_array_equal(gi["end_cost"], ei["end_cost"])
        np.testing.assert_array_equal(gi["best_end"], ei["best_end"])
        for x, y in zip(gi["begins"], ei["begins"]):
            np.testing.assert_array_equal(x, y)
        if want_path:
            for x, y in zip(gi["paths"], ei["paths"]):
                np.testing.assert_array_equal(x, y)
    assert got == dec.decode_batch(own)[0] and any(len(wd) >= 1 for wd in got)
    on.close(); fresh.close(); decoys.close(); own.close()


def test_online_bigram_wide_one_frame_stream_shows_column_zero(hip, ctx):
    """With the FIRST states among the end rows, a stream that holds one frame shows its column 0: init[w] + the frame's
    likelihood of the word's first state, exactly, and +inf in every other state -- on a fresh stream and on one that has
    been reset after taking other frames (the start-row term goes by the absolute column, the carried column is not read)."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(1801)
    W, n = 18, 3
    means, vars_, w = make_model(rng, W, n)
    wt = [word_trans(rng, n) for _ in range(W)]
    B, init = random_costs(rng, W, 0.2)
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    first = 1 + W * (n - 1) + W                                           # state 0 of word w is row first + w
    ends = np.concatenate([np.asarray(graph["end_rows"]), first + np.arange(W)]).astype(np.int32)
    g = dict(graph, end_rows=ends)
    gmm = packed(hip, ctx, means, vars_, w)
    lat = hip.Lattices(ctx, [g])
    assert "bigram_wide" in lat.forms()
    b = hip.Batch(ctx, [rng.normal(size=(9, means.shape[3])) * 2.0, rng.normal(size=(5, means.shape[3])) * 2.0])
    nll = b.loglik(gmm)
    s = hip.OnlineBigramWideSession(ctx, lat, 3, 9)
    s.push(b, [2, 0], first=[0, 0], count=[7, 1])                         # stream 2 takes seven frames, stream 0 one
    s.reset([2])
    s.push(b, [2, 0], first=[8, 1], count=[1, 0])                         # ... and after its reset one, the batch's row 8
    r = s.result([2, 0, 1])
    assert r["frames"].tolist() == [1, 1, 0]
    for k, row in ((0, 8), (1, b.offsets[1])):
        np.testing.assert_array_equal(r["end_cost"][k][:W], np.full(W, np.inf))
        np.testing.assert_array_equal(r["end_cost"][k][W:], init + nll[row, graph["row_state"][first:first + W]])
    assert np.isfinite(r["end_cost"][0][W:]).any() and np.isinf(r["end_cost"][0][W:]).any()
    assert np.all(np.isinf(r["end_cost"][2])) and r["best_end"][2] == -1
    s.close(); b.close(); lat.close(); gmm.close()


# ------------------------------------------------------------------ a 20-word vocabulary with a language model, end to end
W20, N20, M20, D20 = 20, 3, 2, 39
TICK = 20


@pytest.fixture(scope="module")
def model20(R):
    """20 words x 3 states, 39 dimensions (what the audio front-end emits), 12 utterances of 3 to 5 words and a bigram
    model fitted on their word strings."""
    from sr.langmodel import BigramModel
    rng = np.random.default_rng(2004)
    means = rng.normal(size=(W20, N20, M20, D20)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W20, N20, M20, D20))
    w = rng.dirichlet(np.ones(M20), size=(W20, N20))
    trans = [word_trans(rng, N20) for _ in range(W20)]
    hmms = [make_hmm(R, means[i], vars_[i], w[i], trans[i]) for i in range(W20)]
    xs, seqs = [], []
    for u in range(12):
        segs = []
        seqs.append([int(v) for v in rng.integers(0, W20, size=rng.integers(3, 6))])
        for wd in seqs[-1]:
            Tw = int(rng.integers(8, 19))
            st = np.minimum(np.arange(Tw) * N20 // Tw, N20 - 1)
            comp = rng.integers(0, M20, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D20)))
        xs.append(np.concatenate(segs))
    return dict(hmms=hmms, xs=xs, lm=BigramModel(W20, smoothing=0.1).fit(seqs))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_bigram_wide_running_results_equal_decode_batch_of_the_prefix(hip, ctx, model20, dtype):
    """push(ids, chunks) in 20-frame ticks, likelihoods per tick; at EVERY tick words, best_end and begins equal
    decode_batch(prefix, want_times=True).  The likelihoods of a tick and of the prefix come from separate launches over
    batches of other shapes, so the end costs are held to 1e-12 (fp32 likelihoods: 1e-5) -- the tolerances of
    test_gpu_online_wide's twin of this test -- and everything discrete exactly."""
    from sr.recognition.batch import ContinuousDecoder, OnlineBigramDecoder
    xs = model20["xs"]
    dec = ContinuousDecoder(model20["hmms"], grammar="bigram", bigram=model20["lm"], lm_scale=2.0, dtype=dtype, ctx=ctx)
    assert "bigram_wide" in dec.lat.forms()
    on = dec.online_bigram(n_streams=12, max_frames=max(len(x) for x in xs), times=True, wide=True)
    assert type(on) is OnlineBigramDecoder and isinstance(on.session, hip.OnlineBigramWideSession)
    ids = np.random.default_rng(4).permutation(12)
    ticks = -(-max(len(x) for x in xs) // TICK)
    assert ticks >= 2
    for tick in range(1, ticks + 1):
        on.push(ids, [x[(tick - 1) * TICK:tick * TICK] for x in xs])
        b = hip.Batch(ctx, [x[:tick * TICK] for x in xs], dtype=dtype)
        ref_words, ref = dec.decode_batch(b, want_times=True)
        words, info = on.result(ids)
        assert words == ref_words
        np.testing.assert_array_equal(info["best_end"], ref["best_end"])
        for x, y in zip(info["begins"], ref["begins"]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_allclose(info["end_cost"].reshape(-1), ref["end_cost_flat"], rtol=1e-12 if dtype == np.float64 else 1e-5)
        assert info["frames"].tolist() == [min(len(x), tick * TICK) for x in xs]
        b.close()
    assert all(3 <= len(wd) for wd in words)
    fin, _ = on.finish(ids, want_path=True)
    assert fin == words and not on.frames.any()
    on.close()


def test_online_bigram_wide_push_audio_decodes_like_the_one_shot_path(hip, ctx, model20):
    """The 20-word model behind a StreamingFrontend, int16 audio in uneven chunks: the final words (and begins) equal
    decode_batch on features_from_signals(..., normalize=) of the whole signals."""
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    from sr.recognition.batch import ContinuousDecoder
    from test_gpu_audio_capture import burst_signal
    rng = np.random.default_rng(18)
    rate, chunk = 16000, 3200
    sigs = [burst_signal(rng, k, 40, [(k // 4, k // 2), (5 * k // 8, 7 * k // 8)], freq=300.0 + 150 * i, rate=rate)
            for i, k in enumerate([8000, 11111, 14000])]
    norm = feature_stats(sigs, rate)
    dec = ContinuousDecoder(model20["hmms"], grammar="bigram", bigram=model20["lm"], lm_scale=2.0, ctx=ctx)
    b = features_from_signals(sigs, rate, normalize=norm)
    ref_words, ref = dec.decode_batch(b, want_times=True)
    frames = b.lengths.tolist()
    fe = StreamingFrontend(3, rate, normalize=norm, max_chunk=chunk)
    on = dec.online_bigram(3, max_frames=max(frames), frontend=fe, times=True, wide=True)
    assert isinstance(on.session, hip.OnlineBigramWideSession)
    pos = [0, 0, 0]
    while any(p < len(s) for p, s in zip(pos, sigs)):                     # uneven chunks, streams at different rates
        live = [k for k in range(3) if pos[k] < len(sigs[k])]
        cnt = [int(rng.choice([0, 1, 160, 401, 1777, chunk])) for _ in live]
        on.push_audio(live, [sigs[k][pos[k]:pos[k] + c] for k, c in zip(live, cnt)], [pos[k] + c >= len(sigs[k]) for k, c in zip(live, cnt)])
        for k, c in zip(live, cnt):
            pos[k] = min(pos[k] + c, len(sigs[k]))
    assert on.frames.tolist() == frames and fe.samples.tolist() == [len(s) for s in sigs]
    words, info = on.result(np.arange(3))
    assert words == ref_words and all(len(wd) >= 1 for wd in words)
    np.testing.assert_array_equal(info["best_end"], ref["best_end"])
    for x, y in zip(info["begins"], ref["begins"]):
        np.testing.assert_array_equal(x, y)
    on.finish([1])                                                        # frees the id in the front-end too
    assert fe.samples[1] == 0 and on.frames[1] == 0
    b.close(); on.close(); fe.close()


# ----------------------------------------------------------------------------------------------------------------------
# 9. refusals
def test_online_bigram_wide_refusals(R, hip, ctx):
    """Through the real library: the graph forms gh_online_create_bigram_wide does not take (the message names the entry
    point that does), commit / tail / window, and pushes that must move no stream."""
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    rng = np.random.default_rng(32)
    W, n, D = 17, 3, 5
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, False, D=D)
    wt = [word_trans(rng, n) for _ in range(W)]
    Bw, initw = random_costs(rng, W, 0.2)
    # graph forms
    loop_wide = hip.Lattices(ctx, [packed_loop_lattice(wt, n, 0.0)[0]])
    with pytest.raises(hip.Unsupported, match="gh_online_create_wide takes it"):
        hip.OnlineBigramWideSession(ctx, loop_wide, 4, 10)
    loop_wide.close()
    loop_narrow = hip.Lattices(ctx, [packed_loop_lattice(wt[:16], n, 0.0)[0]])
    with pytest.raises(hip.Unsupported, match="gh_online_create takes it"):
        hip.OnlineBigramWideSession(ctx, loop_narrow, 4, 10)
    loop_narrow.close()
    narrow = hip.Lattices(ctx, [packed_bigram_lattice(wt[:16], n, Bw[:16, :16], initw[:16])[0]])
    assert "bigram" in narrow.forms()
    with pytest.raises(hip.Unsupported, match="gh_online_create_bigram takes it"):
        hip.OnlineBigramWideSession(ctx, narrow, 4, 10)
    narrow.close()
    layers = hip.Lattices(ctx, [packed_lattice(wt, n, [list(range(W))] * 2)[0]])
    with pytest.raises(hip.Unsupported, match="K-layer"):
        hip.OnlineBigramWideSession(ctx, layers, 4, 10)
    layers.close()
    beam = hip.Lattices(ctx, [packed_bigram_lattice(wt, n, Bw, initw)[0]])
    beam.set_beam(3)
    with pytest.raises(hip.Unsupported, match="beam"):
        hip.OnlineBigramWideSession(ctx, beam, 4, 10)
    beam.close()
    two = hip.Lattices(ctx, [packed_bigram_lattice(wt, n, Bw, initw)[0], packed_bigram_lattice(wt, n, Bw + 1.0, initw)[0]])
    with pytest.raises(hip.Unsupported, match="several graphs"):
        hip.OnlineBigramWideSession(ctx, two, 4, 10)
    two.close()
    # the settled prefix is not built: refused before any session exists
    for kw in (dict(window=10), dict(max_frames=10, settle=True)):
        with pytest.raises(hip.Unsupported, match="not built yet"):
            dec.online_bigram(4, wide=True, **kw)
    with pytest.raises(hip.Unsupported, match="not in bigram form"):      # ... and without the permission: as before
        dec.online_bigram(4, max_frames=10)
    # the session does not settle
    on = dec.online_bigram(n_streams=3, max_frames=12, times=True, wide=True)
    s = on.session
    assert isinstance(s, hip.OnlineBigramWideSession)
    for call in (s.commit, s.tail):
        with pytest.raises(hip.Unsupported, match="does not settle"):
            call()
    settled = np.zeros(3, dtype=np.int64)
    assert ctx.lib.gh_online_commit(ctx.h, s.h, 3, None, settled.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, None) \
        == hip.GH_ERR_UNSUPPORTED
    assert ctx.lib.gh_online_tail(ctx.h, s.h, 3, None, None, None, None, None, None, None) == hip.GH_ERR_UNSUPPORTED
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(hip.Unsupported):
            call()
    # pushes that are refused as a whole
    xs = [rng.normal(size=(T, D)) * 2.0 for T in (9, 6, 4)]
    on.push([0, 1, 2], xs)
    b = hip.Batch(ctx, [rng.normal(size=(4, D)), rng.normal(size=(3, D))])
    b.loglik(dec.gmm, fetch=False)
    on.push_batch([1, 0], b)                                             # stream 1: 6 + 4, stream 0: 9 + 3 = capacity
    assert s.frames().tolist() == [12, 10, 4] == on.frames.tolist()
    mid = on.result(want_path=True)
    for ids, kw in (([2, 0], {}),                                        # stream 0 is full: stream 2 must not move either
                    ([2, 2], {}), ([2, 3], {}), ([-1, 2], {}),           # an id twice, ids out of range
                    ([2, 1], dict(first=[2, 0], count=[3, 1])),          # columns [2, 5) of a 4-frame utterance
                    ([2, 1], dict(first=[0, -1]))):
        with pytest.raises(hip.BackendError):
            s.push(b, ids, **kw)
        assert s.frames().tolist() == [12, 10, 4]
    after = on.result(want_path=True)
    assert after[0] == mid[0]
    np.testing.assert_array_equal(after[1]["end_cost"], mid[1]["end_cost"])
    np.testing.assert_array_equal(after[1]["best_end"], mid[1]["best_end"])
    for p, q in zip(after[1]["paths"], mid[1]["paths"]):
        np.testing.assert_array_equal(p, q)
    with pytest.raises(ValueError):                                      # the same through the decoder: before the GPU is touched
        on.push([2, 0], [xs[2], xs[2]])
    with pytest.raises(hip.BackendError):
        s.result([3])
    s.push(b, [2, 1], first=[0, 1], count=[4, 2])                        # exactly to capacity is fine
    assert s.frames().tolist() == [12, 12, 8]
    on.close()
    b.close()
