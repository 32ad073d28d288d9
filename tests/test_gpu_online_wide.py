# -*- coding: utf-8 -*-
"""Online decoding for vocabularies of 17 to 64 words on the device (gh_viterbi_online_wide.hip, gh_online_create_wide):
the WIDE loop sweep carried across chunks, one wave per stream.

The contract is "online == offline on the prefix", held against the one-shot wide loop kernel:
  1. the dynamic program alone -- ONE resident likelihood matrix fed in random column ranges -- is BITWISE
     viterbi_loop_wide_kernel on the same matrix: end costs, chosen ends, paths, labels and begins;
  2. the same one frame per push (the column-0 start term and the per-column history address at their smallest);
  3. reused ids: half of another utterance, a reset, then the stream's own, against a fresh session;
  4. running results at every 20-frame tick against decode_batch of the prefix;
  5. audio through a StreamingFrontend;
  6. refusals through the real library: graph forms, commit / tail / window, and pushes that must change nothing."""
import ctypes as C

import numpy as np
import pytest

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


def word_trans(rng, n, skip=False, last_self=0.0):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.05, 0.6) if i < n - 1 else last_self
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.8, 2.5)
        if skip and i < n - 2 and rng.random() < 0.6:
            t[i + 2, i] = rng.uniform(1.5, 4.0)
    return t


def make_hmm(R, means, vars_, w, trans):
    h = R.HMM(means.shape[0])
    h.gmm_states = []
    for s in range(means.shape[0]):
        g = R.GMM(means[s, 0].copy(), vars_[s, 0].copy(), means.shape[1])
        g.update_models(means[s].copy(), vars_[s].copy(), w[s].copy())
        h.gmm_states.append(g)
    h.transitions = trans.copy()
    h.mu, h.sigma = means[:, 0].copy(), vars_[:, 0].copy()
    return h


def make_decoder(R, ctx, rng, W, n, skip, penalty, M=2, D=6, dtype=np.float64):
    from sr.recognition.batch import ContinuousDecoder
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    hmms = [make_hmm(R, means[i], vars_[i], w[i], word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3))) for i in range(W)]
    return ContinuousDecoder(hmms, grammar="loop", word_penalty=penalty, dtype=dtype, ctx=ctx), means, vars_


def make_utts(rng, means, vars_, U, short_every=9, words=(1, 7)):
    """Ragged utterances of random words; every `short_every`-th is noise shorter than any word (>= 2 frames)."""
    W, n, M, D = means.shape
    xs = []
    for u in range(U):
        if short_every and u % short_every == 0:
            xs.append(rng.normal(size=(int(rng.integers(2, max(3, n))), D)) * 2.0)
            continue
        segs = []
        for wd in rng.integers(0, W, size=rng.integers(*words)):
            Tw = int(rng.integers(n, 3 * n + 4))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            comp = rng.integers(0, M, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D)))
        xs.append(np.concatenate(segs))
    return xs


def assert_bitwise_the_one_shot_decode(dec, on, ids, b, n):
    """`on` (times=True) has taken the whole batch `b` on the streams `ids`: everything equals the one-shot wide kernel."""
    row_word = np.where(dec.row_state >= 0, dec.row_state // n, -1).astype(np.int32)
    np.testing.assert_array_equal(on.frames[ids], np.asarray(b.lengths, dtype=np.int64))
    ref = dec.lat.viterbi(b, want_path=True)                            # the one-shot wide loop kernel on the SAME matrix
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


# the wide rows of test_gpu_layers.test_loop_kernel_equals_lean_kernel's list, the smallest word and the most registers
WIDE = [(17, 5, False, 0.5), (40, 3, True, 1.0), (64, 5, False, 0.0), (33, 8, True, 2.0), (17, 2, False, 0.0), (64, 8, True, 1.0)]


@pytest.mark.parametrize("W,n,skip,penalty", WIDE)
def test_online_wide_sweep_is_bitwise_the_wide_loop_kernel(R, hip, ctx, W, n, skip, penalty):
    """The DP yardstick: one whole-utterance batch with resident likelihoods, fed through push_batch(first, count) in
    random column ranges (0- and 1-frame ranges among them), against lat.viterbi / viterbi_labels on the same batch.
    13 ragged utterances, some shorter than a word, on ids scattered over 19 streams; both dtypes."""
    rng = np.random.default_rng(77 * W + n)
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, skip, penalty)
    assert "loop" in dec.lat.forms()
    xs = make_utts(rng, means, vars_, 13)
    for dtype in (np.float64, np.float32):
        b = hip.Batch(ctx, xs, dtype=dtype)
        T = np.asarray(b.lengths, dtype=np.int64)
        on = dec.online(n_streams=19, max_frames=int(T.max()), times=True)
        assert isinstance(on.session, hip.OnlineWideSession)
        ids = rng.permutation(19)[:b.U]
        pos = np.zeros(b.U, dtype=np.int64)
        while np.any(pos < T):
            cnt = np.minimum(rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 1000], size=b.U), T - pos)
            on.push_batch(ids, b, first=pos, count=cnt)                 # (the first call computes the likelihoods, once)
            pos += cnt
        assert_bitwise_the_one_shot_decode(dec, on, ids, b, n)
        on.close()
        b.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_wide_one_frame_at_a_time(R, hip, ctx, dtype):
    """Every stream takes strictly ONE frame per push: the start-row term of column 0 and the history address of every
    single column."""
    W, n = 17, 5
    rng = np.random.default_rng(1705)
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, False, 0.5)
    xs = make_utts(rng, means, vars_, 13)
    b = hip.Batch(ctx, xs, dtype=dtype)
    T = np.asarray(b.lengths, dtype=np.int64)
    on = dec.online(n_streams=19, max_frames=int(T.max()), times=True)
    ids = rng.permutation(19)[:b.U]
    for t in range(int(T.max())):
        on.push_batch(ids, b, first=np.minimum(t, T), count=(t < T).astype(np.int64))
    assert_bitwise_the_one_shot_decode(dec, on, ids, b, n)
    on.close()
    b.close()


@pytest.mark.parametrize("W,n,skip", [(17, 5, False), (40, 3, True)])
def test_online_wide_reused_id_equals_a_fresh_session(R, hip, ctx, W, n, skip):
    """Streams take half of ANOTHER utterance, are reset, and take their own, while one stream sits ticks out: what the
    first utterance left in the carried column and in the history must not show.  Bitwise a fresh session."""
    rng = np.random.default_rng(900 + W)
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, skip, 0.7)
    pool = sorted(make_utts(rng, means, vars_, 7, short_every=0, words=(2, 6)), key=len)
    decoys = hip.Batch(ctx, [pool[-1], pool[-2], pool[3]])
    own = hip.Batch(ctx, [pool[0], pool[1], pool[3]])                       # shorter than the decoys: old history lies behind
    cap = len(pool[-1])
    on = dec.online(n_streams=5, max_frames=cap, times=True)
    half = [len(pool[-1]) // 2, len(pool[-2]) // 2]
    on.push_batch([4, 1, 2], decoys, first=[0, 0, 0], count=half + [3])
    assert on.frames.tolist() == [0, half[1], 3, 0, half[0]]
    on.reset([4, 1])
    assert on.frames.tolist() == [0, 0, 3, 0, 0]
    k = 2
    on.push_batch([4, 1, 2], own, first=[0, 0, 3], count=[k, len(pool[1]), 0])      # stream 2 sits this tick out
    on.push_batch([4, 1, 2], own, first=[k, len(pool[1]), 3], count=[len(pool[0]) - k, 0, len(pool[3]) - 3])
    fresh = dec.online(n_streams=5, max_frames=cap, times=True)
    fresh.push_batch([0, 3, 2], decoys, count=[0, 0, 3])                  # (the same likelihood values as stream 2 above)
    fresh.push_batch([0, 3, 2], own, first=[0, 0, 3])
    for want_path in (False, True):
        got, gi = on.result([4, 1, 2], want_path=want_path)
        exp, ei = fresh.result([0, 3, 2], want_path=want_path)
        assert got == exp and all(len(wd) >= 1 for wd in got)
        np.testing.assert_array_equal(gi["end_cost"], ei["end_cost"])
        np.testing.assert_array_equal(gi["best_end"], ei["best_end"])
        for x, y in zip(gi["begins"], ei["begins"]):
            np.testing.assert_array_equal(x, y)
        if want_path:
            for x, y in zip(gi["paths"], ei["paths"]):
                np.testing.assert_array_equal(x, y)
    assert got == dec.decode_batch(own)[0]
    on.close(); fresh.close(); decoys.close(); own.close()


# ------------------------------------------------------------------ a 20-word vocabulary, end to end
W20, N20, M20, D20 = 20, 3, 2, 39
TICK = 20


@pytest.fixture(scope="module")
def model20(R):
    """20 words x 3 states, 39 dimensions (what the audio front-end emits), and 12 utterances of 3 to 5 words."""
    rng = np.random.default_rng(2003)
    means = rng.normal(size=(W20, N20, M20, D20)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W20, N20, M20, D20))
    w = rng.dirichlet(np.ones(M20), size=(W20, N20))
    trans = [word_trans(rng, N20) for _ in range(W20)]
    hmms = [make_hmm(R, means[i], vars_[i], w[i], trans[i]) for i in range(W20)]
    xs = []
    for u in range(12):
        segs = []
        for wd in rng.integers(0, W20, size=rng.integers(3, 6)):
            Tw = int(rng.integers(8, 19))
            st = np.minimum(np.arange(Tw) * N20 // Tw, N20 - 1)
            comp = rng.integers(0, M20, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D20)))
        xs.append(np.concatenate(segs))
    return dict(hmms=hmms, xs=xs)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_wide_running_results_equal_decode_batch_of_the_prefix(hip, ctx, model20, dtype):
    """push(ids, chunks) in 20-frame ticks, likelihoods per tick; at EVERY tick words, best_end and begins equal
    decode_batch(prefix, want_times=True), end costs to 1e-12 (fp32 likelihoods: 1e-5) -- the tolerances of
    test_online_end_to_end_equals_decode_batch for likelihoods computed separately."""
    from sr.recognition.batch import ContinuousDecoder
    xs = model20["xs"]
    dec = ContinuousDecoder(model20["hmms"], grammar="loop", word_penalty=0.5, dtype=dtype, ctx=ctx)
    assert "loop" in dec.lat.forms()
    on = dec.online(n_streams=12, max_frames=max(len(x) for x in xs), times=True)
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


def test_online_wide_push_audio_decodes_like_the_one_shot_path(hip, ctx, model20):
    """The 20-word model behind a StreamingFrontend, int16 audio in uneven chunks: the final words (and begins) equal
    decode_batch on features_from_signals(..., normalize=) of the whole signals."""
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    from sr.recognition.batch import ContinuousDecoder
    from test_gpu_audio_capture import burst_signal
    rng = np.random.default_rng(17)
    rate, chunk = 16000, 3200
    sigs = [burst_signal(rng, k, 40, [(k // 4, k // 2), (5 * k // 8, 7 * k // 8)], freq=300.0 + 150 * i, rate=rate)
            for i, k in enumerate([8000, 11111, 14000])]
    norm = feature_stats(sigs, rate)
    dec = ContinuousDecoder(model20["hmms"], grammar="loop", word_penalty=0.5, ctx=ctx)
    b = features_from_signals(sigs, rate, normalize=norm)
    ref_words, ref = dec.decode_batch(b, want_times=True)
    frames = b.lengths.tolist()
    fe = StreamingFrontend(3, rate, normalize=norm, max_chunk=chunk)
    on = dec.online(3, max_frames=max(frames), frontend=fe, times=True)
    assert isinstance(on.session, hip.OnlineWideSession)
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


def test_online_wide_refusals(R, hip, ctx):
    """Through the real library: the graph forms gh_online_create_wide does not take (the message names the entry point
    that does), commit / tail / window, and pushes that must move no stream.  The narrow entry point still refuses a
    17-word graph."""
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    rng = np.random.default_rng(31)
    W, n, D = 17, 3, 5
    dec, means, vars_ = make_decoder(R, ctx, rng, W, n, False, 0.0, D=D)
    wt = [m for m in (word_trans(rng, n) for _ in range(W))]
    # graph forms
    narrow = hip.Lattices(ctx, [packed_loop_lattice(wt[:16], n, 0.0)[0]])
    with pytest.raises(hip.Unsupported, match="gh_online_create takes it"):
        hip.OnlineWideSession(ctx, narrow, 4, 10)
    narrow.close()
    layers = hip.Lattices(ctx, [packed_lattice(wt, n, [list(range(W))] * 3)[0]])
    assert "loop" not in layers.forms()
    with pytest.raises(hip.Unsupported, match="K-layer"):
        hip.OnlineWideSession(ctx, layers, 4, 10)
    layers.close()
    bigram = hip.Lattices(ctx, [packed_bigram_lattice(wt[:4], n, rng.uniform(0.5, 3.0, size=(4, 4)), None)[0]])
    with pytest.raises(hip.Unsupported, match="gh_online_create_bigram takes it"):
        hip.OnlineWideSession(ctx, bigram, 4, 10)
    bigram.close()
    beam = hip.Lattices(ctx, [packed_loop_lattice(wt, n, 0.0)[0]])
    beam.set_beam(3)
    with pytest.raises(hip.Unsupported, match="beam"):
        hip.OnlineWideSession(ctx, beam, 4, 10)
    beam.close()
    two = hip.Lattices(ctx, [packed_loop_lattice(wt, n, 0.0)[0], packed_loop_lattice(wt, n, 1.0)[0]])
    with pytest.raises(hip.Unsupported, match="several graphs"):
        hip.OnlineWideSession(ctx, two, 4, 10)
    two.close()
    with pytest.raises(hip.Unsupported):                                  # the narrow entry point: as before
        hip.OnlineSession(ctx, dec.lat, 4, 10)
    with pytest.raises(hip.Unsupported):
        hip.OnlineSession(ctx, dec.lat, 4, window=10)
    with pytest.raises(hip.Unsupported):                                  # ... and no window on a wide decoder
        dec.online(4, window=10)
    # a wide session does not settle
    on = dec.online(n_streams=3, max_frames=12, times=True)
    s = on.session
    assert isinstance(s, hip.OnlineWideSession)
    for call in (s.commit, s.tail):
        with pytest.raises(hip.Unsupported, match="does not settle"):
            call()
    settled = np.zeros(3, dtype=np.int64)
    assert ctx.lib.gh_online_commit(ctx.h, s.h, 3, None, settled.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, None) \
        == hip.GH_ERR_UNSUPPORTED
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
