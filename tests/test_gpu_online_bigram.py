# -*- coding: utf-8 -*-
"""Online decoding with a bigram grammar on the device (gh_viterbi_bigram_online.hip, gh_online_create_bigram): the
bigram-form sweep carried across chunks.

The contract is "online == offline on the prefix", BITWISE on the same likelihood matrix:
  1. the dynamic program alone, for every instantiated word size x skip arcs: one resident likelihood matrix fed in random
     column ranges against the one-shot bigram kernel (end costs, chosen ends, paths, labels, begins: array_equal);
  2. ties between predecessor words, one frame at a time;
  3. a reused stream id (stale open word, stale partial words, stale history behind the new end);
  4. the reference's own G20 decodes in chunks of 1, 7 and 50 frames;
  5. end to end through ContinuousDecoder.online_bigram with a BigramModel, per tick against decode_batch of the prefix;
  6. audio through a StreamingFrontend, and recordings through a StreamingEndpointer;
  7. refusals through the real library."""
import warnings

import numpy as np
import pytest

from conftest import load_golden
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

M, D = 2, 6


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


def word_trans(rng, n, skip=False, last_self=0.0, integer=False):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = (float(rng.integers(0, 2)) if integer else rng.uniform(0.05, 0.6)) if i < n - 1 else last_self
        if i < n - 1:
            t[i + 1, i] = float(rng.integers(1, 3)) if integer else rng.uniform(0.8, 2.5)
        if skip and i < n - 2 and (i == 0 or rng.random() < 0.6):         # (i == 0: every word has a skip arc)
            t[i + 2, i] = float(rng.integers(2, 4)) if integer else rng.uniform(1.5, 4.0)
    return t


def random_costs(rng, W, forbid):
    """B [W, W] with a fraction `forbid` of +inf entries, every word keeping one way in; start costs with some +inf."""
    B = rng.uniform(0.0, 4.0, size=(W, W))
    B[rng.random((W, W)) < forbid] = np.inf
    B[rng.integers(0, W, size=W), np.arange(W)] = rng.uniform(0.0, 4.0, size=W)
    init = rng.uniform(0.0, 2.0, size=W)
    init[rng.random(W) < 0.3] = np.inf
    init[int(rng.integers(0, W))] = rng.uniform(0.0, 2.0)
    return B, init


def make_model(rng, W, n, m=M, d=D):
    means = rng.normal(size=(W, n, m, d)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, m, d))
    w = rng.dirichlet(np.ones(m), size=(W, n))
    return means, vars_, w


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


def make_utts(rng, means, vars_, U, short_every=9, max_words=6):
    W, n, m, d = means.shape
    xs = []
    for u in range(U):
        if short_every and u % short_every == 0:
            xs.append(rng.normal(size=(int(rng.integers(2, max(3, n))), d)) * 2.0)      # shorter than any word
            continue
        segs = []
        for wd in rng.integers(0, W, size=rng.integers(1, max_words + 1)):
            Tw = int(rng.integers(n, 3 * n + 4))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            comp = rng.integers(0, m, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, d)))
        xs.append(np.concatenate(segs))
    return xs


def bigram_decoder(R, ctx, rng, W, n, skip):
    from sr.recognition.batch import ContinuousDecoder
    means, vars_, w = make_model(rng, W, n)
    hmms = [make_hmm(R, means[i], vars_[i], w[i], word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3))) for i in range(W)]
    B, init = random_costs(rng, W, rng.uniform(0.1, 0.3))
    dec = ContinuousDecoder(hmms, grammar="bigram", bigram=B, initial=init, ctx=ctx)
    assert "bigram" in dec.lat.forms()
    return dec, means, vars_


def bigram_cpw(n, skip):
    return 32 // (n + 5 + (n - 2 if skip else 0))


# every word size x skip arcs the carried sweep is instantiated for, W from {2, 5, 11, 16}
SIZES = [(2, False)] + [(n, s) for n in (3, 4, 5, 6, 7, 8, 12) for s in (False, True)] + [(16, False)]
SWEEP = [((2, 5, 11, 16)[(i + (i // 4)) % 4], n, s) for i, (n, s) in enumerate(SIZES)]


assert len(SWEEP) == 16 and {w for w, _, _ in SWEEP} == {2, 5, 11, 16}                  # a full row of 16 words, rows with idle lanes
assert {bigram_cpw(n, s) for _, n, s in SWEEP} == {4, 3, 2, 1}                          # every number of columns per record word
assert any(n <= 8 for _, n, _ in SWEEP) and any(n > 8 for _, n, _ in SWEEP)             # both ring depths


@pytest.mark.parametrize("W,n,skip", SWEEP)
def test_online_bigram_sweep_is_bitwise_the_bigram_kernel(R, hip, ctx, W, n, skip):
    """The DP yardstick: one whole-utterance batch with resident likelihoods, fed through push_batch(first, count) in
    random column ranges (0- and 1-frame ranges, ranges that end inside a record word), against lat.viterbi /
    viterbi_labels on the same batch.  41 ragged utterances of >= 2 frames, some shorter than any word (an all-+inf end:
    the back-trace's fallback arcs); ids scattered over 47 streams."""
    rng = np.random.default_rng(5000 + 100 * W + 2 * n + skip)
    dec, means, vars_ = bigram_decoder(R, ctx, rng, W, n, skip)
    xs = make_utts(rng, means, vars_, 41)
    assert min(len(x) for x in xs) >= 2
    row_word = np.where(dec.row_state >= 0, dec.row_state // n, -1).astype(np.int32)
    for dtype in (np.float64, np.float32):
        b = hip.Batch(ctx, xs, dtype=dtype)
        T = np.asarray(b.lengths, dtype=np.int64)
        on = dec.online_bigram(n_streams=47, max_frames=int(T.max()), times=True)
        ids = rng.permutation(47)[:b.U]
        assert b.U % 4 != 0 and on.n_streams % 4 != 0
        pos = np.zeros(b.U, dtype=np.int64)
        while np.any(pos < T):
            cnt = np.minimum(rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 1000], size=b.U), T - pos)
            on.push_batch(ids, b, first=pos, count=cnt)                 # (the first call computes the likelihoods, once)
            pos += cnt
        np.testing.assert_array_equal(on.frames[ids], T)
        ref = dec.lat.viterbi(b, want_path=True)                        # the one-shot bigram kernel on the SAME matrix
        words, info = on.result(ids, want_path=True)
        np.testing.assert_array_equal(info["end_cost"].reshape(-1), ref["end_cost_flat"])
        np.testing.assert_array_equal(info["best_end"], ref["best_end"])
        assert np.isfinite(ref["end_cost_flat"]).any()
        if not skip and n > 2:
            assert any(not np.isfinite(ref["end_cost"][u]).any() for u in range(b.U)), "utterances that no word fits are part of the plan"
        for u in range(b.U):
            np.testing.assert_array_equal(info["paths"][u], ref["paths"][u])
        lab = dec.lat.viterbi_labels(b, row_word, max_labels=dec._max_labels(b.lengths), want_begin=True)
        words2, info2 = on.result(ids)
        assert words2 == [[int(v) for v in l] for l in lab["labels"]] == words
        for u in range(b.U):
            np.testing.assert_array_equal(info2["begins"][u], lab["begins"][u])
            np.testing.assert_array_equal(info["begins"][u], lab["begins"][u])     # (the host rule on the path)
        np.testing.assert_array_equal(info2["end_cost"].reshape(-1), ref["end_cost_flat"])
        np.testing.assert_array_equal(info2["best_end"], ref["best_end"])
        on.close()
        b.close()


def dense_of(graph):
    Rr = len(graph["row_state"])
    t = np.full((Rr, Rr), np.inf)
    t[graph["arc_to"], graph["arc_from"]] = graph["arc_cost"]
    return t


def test_online_bigram_breaks_ties_like_the_one_shot_kernel(hip, ctx):
    """The model of test_gpu_bigram.test_bigram_kernel_breaks_ties_like_the_reference (word models in identical pairs, small
    integer costs), pushed ONE FRAME AT A TIME through the binding: paths equal the one-shot kernel's, and entry-row cells
    with two equal best predecessors lie on them."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(4242)
    W, n, m, d = 8, 3, 1, 4
    half = make_model(rng, W // 2, n, m, d)
    means, vars_, w = (np.repeat(a, 2, axis=0) for a in half)
    t1 = [word_trans(rng, n, integer=True) for _ in range(W // 2)]
    wt = [t1[i // 2] for i in range(W)]
    B = np.repeat(rng.integers(0, 4, size=(W // 2, W)).astype(np.float64), 2, axis=0)
    init = np.repeat(rng.integers(0, 3, size=W // 2), 2).astype(np.float64)
    xs = make_utts(rng, means, vars_, 30, short_every=0)
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, m, d), vars_.reshape(W * n, m, d), w.reshape(W * n, m))
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    lat = hip.Lattices(ctx, [graph])
    assert "bigram" in lat.forms()
    b = hip.Batch(ctx, xs)
    nll = b.loglik(gmm)
    ref = lat.viterbi(b, want_path=True)
    T = np.asarray(b.lengths, dtype=np.int64)
    s = hip.OnlineBigramSession(ctx, lat, b.U, int(T.max()))
    ids = np.arange(b.U)[::-1].copy()
    for t in range(int(T.max())):
        s.push(b, ids, first=np.minimum(t, T), count=(t < T).astype(np.int64))
    r = s.result(ids, want_path=True)
    np.testing.assert_array_equal(r["end_cost"].reshape(-1), ref["end_cost_flat"])
    np.testing.assert_array_equal(r["best_end"], ref["best_end"])
    dense = dense_of(graph)
    nes = graph["row_state"] < 0
    first = 1 + W * (n - 1)
    ties_on_path = 0
    for u in range(b.U):
        np.testing.assert_array_equal(r["paths"][u], ref["paths"][u])
        E = np.zeros((len(nes), T[u]))
        E[~nes] = nll[b.offsets[u]:b.offsets[u + 1]][:, graph["row_state"][~nes]].T
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            costs, _ = O.decode_states(E, nes, dense, end_points=[[int(e), -1] for e in graph["end_rows"]])
        for row, col in r["paths"][u]:
            if first <= row < first + W:
                cand = dense[row] + costs[:, col]
                ties_on_path += int(np.sum(cand == cand.min()) > 1)
    assert ties_on_path >= 10, ties_on_path
    s.close(); b.close(); lat.close(); gmm.close()


@pytest.mark.parametrize("n,skip", [(5, False), (3, True), (12, False)])
def test_online_bigram_reused_id_equals_a_fresh_session(R, hip, ctx, n, skip):
    """A stream is finished and its id takes a different, SHORTER utterance while another stream sits a tick out: what is
    left of the first utterance (its open word, its left-aligned partial words, its history behind the new end) must not
    show.  The result equals that of a fresh session, bit for bit."""
    rng = np.random.default_rng(600 + n)
    W = 5
    dec, means, vars_ = bigram_decoder(R, ctx, rng, W, n, skip)
    cpw = bigram_cpw(n, skip)
    pool = sorted(make_utts(rng, means, vars_, 8, short_every=0, max_words=6), key=len)
    long_, other = pool[-1], pool[-2]
    short = make_utts(rng, means, vars_, 1, short_every=0, max_words=2)[0][:len(long_) - cpw - 1]
    assert 2 <= len(short) < len(long_) and len(other) > 3
    cap = len(long_)
    on = dec.online_bigram(n_streams=3, max_frames=cap, times=True)
    one = hip.Batch(ctx, [long_, other])
    cut = len(long_) - 1 if cpw == 1 else (len(long_) // cpw) * cpw - 1      # (cpw > 1: the first push ends inside a word)
    on.push_batch([2, 0], one, first=[0, 0], count=[cut, 3])
    on.push_batch([2, 0], one, first=[cut, 3], count=[len(long_) - cut, 0])   # stream 0 sits this tick out
    w_long, _ = on.finish([2])
    assert on.frames.tolist() == [3, 0, 0]
    two = hip.Batch(ctx, [short, other])
    k = min(len(short) - 1, cpw + 1)
    on.push_batch([2, 0], two, first=[0, 3], count=[k, 0])                    # ... and this one
    on.push_batch([2, 0], two, first=[k, 3], count=[len(short) - k, len(other) - 3])
    fresh = dec.online_bigram(n_streams=3, max_frames=cap, times=True)
    fresh.push_batch([1, 2], two)
    for want_path in (False, True):
        got, gi = on.result([2, 0], want_path=want_path)
        exp, ei = fresh.result([1, 2], want_path=want_path)
        assert got == exp
        np.testing.assert_array_equal(gi["end_cost"], ei["end_cost"])
        np.testing.assert_array_equal(gi["best_end"], ei["best_end"])
        for x, y in zip(gi["begins"], ei["begins"]):
            np.testing.assert_array_equal(x, y)
        if want_path:
            for x, y in zip(gi["paths"], ei["paths"]):
                np.testing.assert_array_equal(x, y)
    ref_words, ref = dec.decode_batch(two, want_times=True)
    assert got == ref_words and len(w_long[0]) >= 1
    on.close(); fresh.close(); one.close(); two.close()


@pytest.mark.parametrize("chunk", [1, 7, 50])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_bigram_G20_in_chunks(R, hip, ctx, dtype, chunk):
    """G20 (the reference's own decode of the bigram graph: random, forbidden and tied costs), its utterances taken `chunk`
    frames at a time: paths BIT-EXACT to the golden, end costs 1e-10 (fp32 likelihoods: 1e-5), digits equal."""
    from sr.recognition.batch import ContinuousDecoder
    g = load_golden("G20_bigram_grammar")
    U = int(g["n_utts"])
    for case in range(int(g["n_cases"])):
        pp = "c%d_" % case
        means, vars_, w = g[pp + "means"], g[pp + "vars"], g[pp + "w"]
        hmms = [make_hmm(R, means[i], vars_[i], w[i], g["word_trans"]) for i in range(means.shape[0])]
        dec = ContinuousDecoder(hmms, grammar="bigram", bigram=g[pp + "B"], initial=g[pp + "init"], dtype=dtype, ctx=ctx)
        assert "bigram" in dec.lat.forms()
        xs = [g[pp + "x%d" % u] for u in range(U)]
        on = dec.online_bigram(n_streams=U, max_frames=max(len(x) for x in xs))
        for t in range(0, max(len(x) for x in xs), chunk):
            on.push(np.arange(U), [x[t:t + chunk] for x in xs])
        words, info = on.result(want_path=True)
        ends = np.asarray(dec.lat.end_rows[0])
        rw = g[pp + "row_word"]
        for u in range(U):
            want = g[pp + "costs%d" % u][ends, -1]
            fin = np.isfinite(want)
            np.testing.assert_array_equal(np.isfinite(info["end_cost"][u]), fin)
            np.testing.assert_allclose(info["end_cost"][u][fin], want[fin], rtol=1e-10 if dtype == np.float64 else 1e-5)
            np.testing.assert_array_equal(info["paths"][u], g[pp + "path%d" % u])
            assert O.path_to_words(info["paths"][u], rw < 0, rw) == list(g[pp + "digits%d" % u]) == words[u]
        assert on.result()[0] == words
        on.close()


def test_online_bigram_end_to_end_with_a_language_model(R, hip, ctx):
    """ContinuousDecoder(grammar="bigram", bigram=BigramModel, lm_scale=) -> online_bigram(times=True): feature chunks per
    tick through `push`; at every tick with >= 2 frames words, begins and best ends equal decode_batch of the prefix;
    `finish` frees the id."""
    from sr.langmodel import BigramModel
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(81)
    W, n, TICK = 4, 3, 5
    means, vars_, w = make_model(rng, W, n)
    hmms = [make_hmm(R, means[i], vars_[i], w[i], word_trans(rng, n)) for i in range(W)]
    lm = BigramModel(W, smoothing=0).fit([[0, 1, 2], [1, 2, 3], [0, 1], [2, 3, 0, 1]])       # unseen pairs are forbidden
    dec = ContinuousDecoder(hmms, grammar="bigram", bigram=lm, lm_scale=2.0, ctx=ctx)
    assert "bigram" in dec.lat.forms()
    xs = make_utts(rng, means, vars_, 6, short_every=0, max_words=4)
    on = dec.online_bigram(n_streams=7, max_frames=max(len(x) for x in xs), times=True)
    ids = np.array([6, 0, 3, 1, 5, 2])
    checked = 0
    for tick in range(1, -(-max(len(x) for x in xs) // TICK) + 1):
        on.push(ids, [x[(tick - 1) * TICK:tick * TICK] for x in xs])
        b = hip.Batch(ctx, [x[:tick * TICK] for x in xs])
        ref_words, ref = dec.decode_batch(b, want_times=True)
        words, info = on.result(ids)
        assert words == ref_words
        np.testing.assert_array_equal(info["best_end"], ref["best_end"])
        np.testing.assert_allclose(info["end_cost"].reshape(-1), ref["end_cost_flat"], rtol=1e-12)
        for x, y in zip(info["begins"], ref["begins"]):
            np.testing.assert_array_equal(x, y)
        assert info["frames"].tolist() == [min(tick * TICK, len(x)) for x in xs]
        checked += 1
        b.close()
    assert checked >= 3 and any(len(wd) >= 2 for wd in words)
    _, B = lm.costs()
    assert all(np.isfinite(B[a, c]) for wd in words for a, c in zip(wd[:-1], wd[1:]))
    fw, fi = on.finish([3])
    assert fw == [words[2]] and on.frames[3] == 0 and on.frames[6] == len(xs[0])
    on.push([3], [xs[1]])                                                 # the id is free: another utterance
    b = hip.Batch(ctx, [xs[1]])
    assert on.result([3])[0] == dec.decode_batch(b)[0]
    b.close()
    on.close()


# ------------------------------------------------------------------ audio in, words out
TICK = 3200


@pytest.fixture(scope="module")
def audio_model(R, ctx):
    """The 39-dimensional 3-word model of test_gpu_stream_frontend.py's `e2e` fixture, under a bigram grammar."""
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(17)
    W, n, m, d = 3, 4, 2, 39
    trans = np.full((n, n), np.inf)
    for i in range(n):
        trans[i, i] = -np.log(0.8) if i < n - 1 else 0.0
        if i < n - 1:
            trans[i + 1, i] = -np.log(0.2)
    hmms = [make_hmm(R, rng.normal(size=(n, m, d)), rng.uniform(0.5, 1.5, size=(n, m, d)), rng.dirichlet(np.ones(m), size=n), trans)
            for _ in range(W)]
    B = np.array([[1.0, 0.5, np.inf], [2.0, 1.0, 0.25], [0.5, np.inf, 1.5]])
    return ContinuousDecoder(hmms, grammar="bigram", bigram=B, initial=[0.0, 1.0, 0.5], ctx=ctx)


def ticks_of(sigs, tick=TICK):
    for t in range(max(-(-len(s) // tick) for s in sigs)):
        live = [k for k, s in enumerate(sigs) if t * tick < len(s)]
        yield live, [sigs[k][t * tick:(t + 1) * tick] for k in live], [(t + 1) * tick >= len(sigs[k]) for k in live]


def test_online_bigram_push_audio_decodes_like_the_one_shot_path(hip, ctx, audio_model):
    """The three shortest signals of test_gpu_stream_frontend.py's end-to-end case through a StreamingFrontend in uneven
    chunks: words and begins equal decode_batch on features_from_signals(..., normalize=) of the whole signals."""
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    from test_gpu_audio_capture import burst_signal
    rng = np.random.default_rng(17)
    rate = 16000
    sigs = [burst_signal(rng, k, 40, [(k // 4, k // 2), (5 * k // 8, 7 * k // 8)], freq=300.0 + 150 * i, rate=rate)
            for i, k in enumerate([8000, 11111, 14000])]
    norm = feature_stats(sigs, rate)
    dec = audio_model
    b = features_from_signals(sigs, rate, normalize=norm)
    ref_words, ref = dec.decode_batch(b, want_times=True)
    frames = b.lengths.tolist()
    fe = StreamingFrontend(3, rate, normalize=norm, max_chunk=TICK)
    on = dec.online_bigram(3, max_frames=max(frames), frontend=fe, times=True)
    pos = [0, 0, 0]
    while any(p < len(s) for p, s in zip(pos, sigs)):                     # uneven chunks, streams at different rates
        live = [k for k in range(3) if pos[k] < len(sigs[k])]
        cnt = [int(rng.choice([0, 1, 160, 401, 1777, TICK])) for _ in live]
        on.push_audio(live, [sigs[k][pos[k]:pos[k] + c] for k, c in zip(live, cnt)], [pos[k] + c >= len(sigs[k]) for k, c in zip(live, cnt)])
        for k, c in zip(live, cnt):
            pos[k] = min(pos[k] + c, len(sigs[k]))
    assert on.frames.tolist() == frames and fe.samples.tolist() == [len(s) for s in sigs]
    words, info = on.result(np.arange(3))
    assert words == ref_words and all(len(wd) >= 1 for wd in words)
    np.testing.assert_array_equal(info["best_end"], ref["best_end"])
    np.testing.assert_allclose(info["end_cost"].reshape(-1), ref["end_cost_flat"], rtol=1e-12)
    for x, y in zip(info["begins"], ref["begins"]):
        np.testing.assert_array_equal(x, y)
    on.finish([1])                                                        # frees the id in the front-end too
    assert fe.samples[1] == 0 and on.frames[1] == 0
    b.close(); on.close(); fe.close()


def test_online_bigram_push_recording_decodes_like_the_offline_path(hip, ctx, audio_model):
    """Two of test_gpu_stream_endpoints.py's two-burst recordings (the second ends while speech is open) through a
    StreamingEndpointer: the utterances equal offline trim_ranges + decode_batch -- ranges, words and word begins."""
    import sr.audio_capture as AC
    import stream_endpoints_ref as S
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    rng = np.random.default_rng(17)
    rate = 16000
    lens = [42000, 43333, 45000, 46111, 48000, 36000]                     # (that test's six draws, of which two are used)
    six = [S.burst_signal(rng, k, 40, [(4000, 10000), (24000, 30000)], freq=300.0 + 150 * i, rate=rate) for i, k in enumerate(lens)]
    six[5] = S.burst_signal(rng, lens[5], 40, [(4000, 10000), (24000, 36000)], rate=rate)        # speech up to the end
    sigs = [six[0], six[5]]
    norm = feature_stats(sigs, rate)
    dec = audio_model
    cfg = AC.default_config(rate)
    det = AC.detect_endpoints(sigs, dict(cfg), max_segments=8)
    assert det["n_segments"].tolist() == [2, 2] and det["open"].tolist() == [False, True]
    begin, stop = AC.trim_ranges(det, [len(x) for x in sigs], dict(cfg))
    offline, longest = [[], []], 0
    for r, bg, e in zip(np.repeat(np.arange(2), det["n_segments"]), begin, stop):
        batch = features_from_signals([sigs[r][bg:e]], rate, normalize=norm)
        words, info = dec.decode_batch(batch, want_times=True)
        offline[r].append((int(bg), int(e), bool(det["open"][r]) and len(offline[r]) == 1, words[0], [int(v) for v in info["begins"][0]]))
        longest = max(longest, int(batch.lengths[0]))
        batch.close()
    ep = AC.StreamingEndpointer(2, cfg, max_chunk=TICK)
    fe = StreamingFrontend(2, rate, normalize=norm, max_chunk=ep.max_piece)
    on = dec.online_bigram(2, max_frames=longest, frontend=fe, endpointer=ep, times=True)
    got = [[], []]
    for ids, chunks, end in ticks_of(sigs):
        for u in on.push_recording(ids, chunks, end):
            got[u["stream"]].append(u)
    for r in range(2):
        assert [(u["begin"], u["stop"], u["open"], u["words"], u["begins"]) for u in got[r]] == offline[r], r
        assert all(len(u["words"]) >= 1 for u in got[r])
        assert all(u["word_begin"] == [u["begin"] + bb * fe.step for bb in u["begins"]] for u in got[r])
    assert on.frames.tolist() == [0, 0] and ep.samples.tolist() == [len(s) for s in sigs]
    on.close(); fe.close(); ep.close()


def test_online_bigram_refusals(R, hip, ctx):
    """Through the real library: gh_online_create_bigram refuses a loop graph, a K-layer graph, a beam and 16 states with
    skip arcs; a push past max_frames or with an id twice is refused as a whole and changes nothing; commit / tail raise
    Unsupported; the loop entry points still refuse the bigram graph."""
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    rng = np.random.default_rng(3)
    W, n = 4, 3
    dec, means, vars_ = bigram_decoder(R, ctx, rng, W, n, False)
    wt = [word_trans(rng, n) for _ in range(W)]
    B, init = random_costs(rng, W, 0.2)
    wt16 = [word_trans(rng, 16, True) for _ in range(2)]
    for graph in (packed_loop_lattice(wt, n, 0.0)[0], packed_lattice(wt, n, [list(range(W))] * 3)[0],
                  packed_bigram_lattice(wt16, 16, np.ones((2, 2)), None)[0]):                 # 16 states with skip arcs
        lat = hip.Lattices(ctx, [graph])
        assert "bigram" not in lat.forms()
        with pytest.raises(hip.Unsupported):
            hip.OnlineBigramSession(ctx, lat, 4, 10)
        lat.close()
    lat = hip.Lattices(ctx, [packed_bigram_lattice(wt, n, B, init)[0]])
    assert "bigram" in lat.forms()
    with pytest.raises(hip.Unsupported):                                  # the loop entry points keep refusing it
        hip.OnlineSession(ctx, lat, 4, 10)
    with pytest.raises(hip.Unsupported):
        hip.OnlineSession(ctx, lat, 4, window=10)
    hip.OnlineBigramSession(ctx, lat, 4, 10).close()
    lat.set_beam(3)
    with pytest.raises(hip.Unsupported):
        hip.OnlineBigramSession(ctx, lat, 4, 10)
    lat.close()
    with pytest.raises(hip.Unsupported):
        dec.online(4, 10)
    on = dec.online_bigram(n_streams=3, max_frames=12)
    xs = [rng.normal(size=(T, D)) * 2.0 for T in (9, 6, 4)]
    on.push([0, 1, 2], xs)
    b = hip.Batch(ctx, [rng.normal(size=(4, D)), rng.normal(size=(3, D))])
    b.loglik(dec.gmm, fetch=False)
    s = on.session                                                       # the binding itself: no Python-side checks
    on.push_batch([1, 0], b)                                             # stream 1: 6 + 4, stream 0: 9 + 3 = capacity
    assert s.frames().tolist() == [12, 10, 4] == on.frames.tolist()
    mid = on.result(want_path=True)
    for ids, kw in (([2, 0], {}),                                        # stream 0 is full: stream 2 must not move either
                    ([2, 2], {}), ([2, 3], {}), ([-1, 2], {}),           # an id twice, ids out of range
                    ([2, 1], dict(first=[2, 0], count=[3, 1]))):         # columns [2, 5) of a 4-frame utterance
        with pytest.raises(hip.BackendError):
            s.push(b, ids, **kw)
        assert s.frames().tolist() == [12, 10, 4]
    with pytest.raises(ValueError):                                      # the same through the decoder: before the GPU is touched
        on.push([2, 0], [xs[2], xs[2]])
    after = on.result(want_path=True)
    assert after[0] == mid[0]
    np.testing.assert_array_equal(after[1]["end_cost"], mid[1]["end_cost"])
    for p, q in zip(after[1]["paths"], mid[1]["paths"]):
        np.testing.assert_array_equal(p, q)
    row_word = np.where(dec.row_state >= 0, dec.row_state // n, -1).astype(np.int32)
    for call in (s.commit, s.tail):                                      # the class ...
        with pytest.raises(hip.Unsupported):
            call([0], row_label=row_word)
    for call in (hip.OnlineSession.commit, hip.OnlineSession.tail):      # ... and the library behind it
        with pytest.raises(hip.BackendError, match="bigram"):
            call(s, [0], row_label=row_word)
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(hip.Unsupported):
            call([0])
    assert s.frames().tolist() == [12, 10, 4]
    s.push(b, [2, 1], first=[0, 1], count=[4, 2])                        # exactly to capacity is fine
    assert s.frames().tolist() == [12, 12, 8]
    on.close()
    b.close()
