# -*- coding: utf-8 -*-
"""Online decoding on the device (gh_viterbi_online.hip, gh_online_*): the loop-grammar sweep carried across chunks.

The contract is "online == offline on the prefix":
  1. the dynamic program alone -- ONE resident likelihood matrix fed in random column ranges -- is BITWISE the one-shot
     loop kernel on the same matrix (end costs array_equal, chosen ends, paths, labels);
  2. end to end (frames in, 20-frame ticks, likelihoods per tick, shuffled ids, streams at different rates, resets and
     reused ids) it gives what `ContinuousDecoder.decode_batch` gives on the whole utterances;
  3. at tick boundaries the running result is `decode_batch` of the prefix;
  4. the reference's own G14 decodes come out in chunks of 1, 7 and 50 frames;
  5. capacity and graph-form errors through the real library: a refused push changes nothing."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import ref_numpy as O

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


# the narrow rows (up to 16 words) of test_gpu_layers.test_loop_kernel_equals_lean_kernel's list
NARROW = [(10, 5, False, 0.0), (11, 5, False, 2.5), (1, 2, False, 0.0), (16, 3, True, 1.0), (5, 8, True, 0.0), (7, 4, False, 0.7),
          (3, 6, True, 3.0), (2, 7, False, 0.0), (4, 12, False, 0.5), (3, 12, True, 1.0), (5, 16, False, 0.0), (2, 16, True, 2.0)]


@pytest.mark.parametrize("W,n,skip,penalty", NARROW)
def test_online_sweep_is_bitwise_the_loop_kernel(R, hip, ctx, W, n, skip, penalty):
    """The DP yardstick: one whole-utterance batch with resident likelihoods, fed through push_batch(first, count) in
    random column ranges (0- and 1-frame ranges among them, ranges that end inside a decision word), against
    lat.viterbi on the same batch.  Ragged utterances, some shorter than a word; 61 streams with ids scattered over 67."""
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(77 * W + n)
    M, D = 2, 6
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    hmms = [make_hmm(R, means[i], vars_[i], w[i], word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3))) for i in range(W)]
    xs = []
    for u in range(61):
        if u % 9 == 0:
            xs.append(rng.normal(size=(int(rng.integers(2, max(3, n))), D)) * 2.0)      # shorter than any word
            continue
        segs = []
        for wd in rng.integers(0, W, size=rng.integers(1, 7)):
            Tw = int(rng.integers(n, 3 * n + 4))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            comp = rng.integers(0, M, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D)))
        xs.append(np.concatenate(segs))
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=penalty, ctx=ctx)
    assert "loop" in dec.lat.forms()
    row_word = np.where(dec.row_state >= 0, dec.row_state // n, -1).astype(np.int32)
    for dtype in (np.float64, np.float32):
        b = hip.Batch(ctx, xs, dtype=dtype)
        T = np.asarray(b.lengths, dtype=np.int64)
        on = dec.online(n_streams=67, max_frames=int(T.max()))
        ids = rng.permutation(67)[:b.U]
        assert b.U % 4 != 0
        pos = np.zeros(b.U, dtype=np.int64)
        while np.any(pos < T):
            cnt = np.minimum(rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 1000], size=b.U), T - pos)
            on.push_batch(ids, b, first=pos, count=cnt)                 # (the first call computes the likelihoods, once)
            pos += cnt
        np.testing.assert_array_equal(on.frames[ids], T)
        ref = dec.lat.viterbi(b, want_path=True)                        # the one-shot loop kernel on the SAME matrix
        words, info = on.result(ids, want_path=True)
        np.testing.assert_array_equal(info["end_cost"].reshape(-1), ref["end_cost_flat"])
        np.testing.assert_array_equal(info["best_end"], ref["best_end"])
        assert np.isfinite(ref["end_cost_flat"]).any()
        for u in range(b.U):
            np.testing.assert_array_equal(info["paths"][u], ref["paths"][u])
        lab = dec.lat.viterbi_labels(b, row_word)
        words2, info2 = on.result(ids)
        assert words2 == [[int(v) for v in l] for l in lab["labels"]] == words
        np.testing.assert_array_equal(info2["end_cost"].reshape(-1), ref["end_cost_flat"])
        on.close()
        b.close()


# ------------------------------------------------------------------------------------------- configs[4], end to end
K, W5, N5, M5, D5 = 7, 10, 5, 8, 39
U_BASE = 800
TICK = 20


@pytest.fixture(scope="module")
def c5(R, ctx):
    """The model and the 800 seven-word utterances of tests/test_gpu_c5.py's recipe."""
    import bench
    rng = np.random.default_rng(1005)
    wl = bench.synth_workload(1005, 1, W=W5, n=N5, M=M5, D=D5)
    means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
    words = rng.integers(0, W5, size=(U_BASE, K))
    Tw = rng.integers(30, 61, size=(U_BASE, K))
    seg_len = Tw.reshape(-1)
    seg_off = np.concatenate([[0], np.cumsum(seg_len)])
    Nb = int(seg_off[-1])
    seg = np.repeat(np.arange(len(seg_len)), seg_len)
    t = np.arange(Nb) - seg_off[seg]
    st = np.minimum(t * N5 // seg_len[seg], N5 - 1)
    idx = (words.reshape(-1)[seg] * N5 + st) * M5 + rng.integers(0, M5, size=Nb)
    X = means.reshape(-1, D5)[idx] + np.sqrt(vars_).reshape(-1, D5)[idx] * rng.standard_normal((Nb, D5))
    off = np.concatenate([[0], np.cumsum(Tw.sum(axis=1))]).astype(np.int64)
    hmms = [make_hmm(R, means[i], vars_[i], wl["w"][i], trans) for i in range(W5)]
    return dict(hmms=hmms, xs=[X[off[u]:off[u + 1]] for u in range(U_BASE)], words=words)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_end_to_end_equals_decode_batch(hip, ctx, c5, dtype):
    """800 streams in 20-frame ticks through push(ids, chunks): shuffled id order, streams that sit ticks out and so
    progress at different rates, 60 streams reset half-way through ANOTHER utterance and their id reused.  After the last
    tick: labels, best_end and paths == decode_batch(want_path=True) on the whole utterances, end costs 1e-12 (fp32
    likelihoods: 1e-5)."""
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(5)
    xs = c5["xs"]
    dec = ContinuousDecoder(c5["hmms"], grammar="loop", dtype=dtype, ctx=ctx)
    on = dec.online(n_streams=U_BASE, max_frames=max(len(x) for x in xs))
    stream_of = rng.permutation(U_BASE)                                   # utterance u lives on stream stream_of[u]
    pos = np.zeros(U_BASE, dtype=np.int64)
    # the reused ids: these streams first take half of some other utterance, are reset, and start their own
    decoy = {int(u): int(rng.integers(0, U_BASE)) for u in rng.choice(U_BASE, size=60, replace=False)}
    decoy_pos = {u: 0 for u in decoy}
    ticks = sat_out = 0
    while np.any(pos < np.array([len(x) for x in xs])):
        live = [u for u in range(U_BASE) if pos[u] < len(xs[u])]
        order = rng.permutation(live)
        ids, chunks = [], []
        for u in order:
            u = int(u)
            r = rng.random()
            if r < 0.15:
                sat_out += 1
                continue                                                  # not part of this tick's push
            if r < 0.25:
                ids.append(stream_of[u]); chunks.append(np.zeros((0, D5)))  # part of it with no frames
                continue
            if u in decoy:
                x = xs[decoy[u]]
                c = x[decoy_pos[u]:decoy_pos[u] + TICK]
                decoy_pos[u] += len(c)
                ids.append(stream_of[u]); chunks.append(c)
                continue
            c = xs[u][pos[u]:pos[u] + TICK]
            pos[u] += len(c)
            ids.append(stream_of[u]); chunks.append(c)
        on.push(ids, chunks)
        ticks += 1
        half = [u for u in decoy if decoy_pos[u] >= len(xs[decoy[u]]) // 2]
        if half:
            assert np.all(on.frames[stream_of[half]] > 0)
            on.reset(stream_of[half])
            assert np.all(on.frames[stream_of[half]] == 0)
            for u in half:
                del decoy[u]
        assert ticks < 400
    assert not decoy and sat_out > 0
    np.testing.assert_array_equal(on.frames[stream_of], [len(x) for x in xs])
    b = hip.Batch(ctx, xs, dtype=dtype)
    ref_words, ref = dec.decode_batch(b, want_path=True)
    words, info = on.result(stream_of, want_path=True)
    assert words == ref_words
    np.testing.assert_array_equal(info["best_end"], ref["best_end"])
    for p, q in zip(info["paths"], ref["paths"]):
        np.testing.assert_array_equal(p, q)
    np.testing.assert_allclose(info["end_cost"].reshape(-1), ref["end_cost_flat"], rtol=1e-12 if dtype == np.float64 else 1e-5)
    lab_words, _ = on.finish(stream_of)                                   # label mode of the back-trace, then all ids free
    assert lab_words == ref_words == dec.decode_batch(b)[0]
    assert not on.frames.any()
    truth = [list(map(int, w)) for w in c5["words"]]
    assert np.mean([a == t for a, t in zip(words, truth)]) > 0.9
    b.close()
    on.close()


def test_online_prefix_property(hip, ctx, c5):
    """16 streams, three tick boundaries each: result() == decode_batch of the frames pushed so far (words, best_end)."""
    from sr.recognition.batch import ContinuousDecoder
    xs = c5["xs"][:16]
    dec = ContinuousDecoder(c5["hmms"], grammar="loop", word_penalty=1.5, ctx=ctx)
    on = dec.online(n_streams=16, max_frames=max(len(x) for x in xs))
    ids = np.arange(16)[::-1].copy()
    checked = 0
    for tick in range(1, 11):
        on.push(ids, [x[(tick - 1) * TICK:tick * TICK] for x in xs])
        if tick in (2, 5, 10):
            b = hip.Batch(ctx, [x[:tick * TICK] for x in xs])
            ref_words, ref = dec.decode_batch(b)
            words, info = on.result(ids)
            assert words == ref_words
            np.testing.assert_array_equal(info["best_end"], ref["best_end"])
            np.testing.assert_allclose(info["end_cost"].reshape(-1), ref["end_cost_flat"], rtol=1e-12)
            assert info["frames"].tolist() == [tick * TICK] * 16 and min(len(x) for x in xs) >= tick * TICK
            b.close()
            checked += 1
    assert checked == 3
    on.close()


@pytest.mark.parametrize("chunk", [1, 7, 50])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_G14_in_chunks(R, hip, ctx, dtype, chunk):
    """G14 (the reference's own decode of the loop graph), its utterances taken `chunk` frames at a time: paths BIT-EXACT
    to the golden, end costs 1e-10 (fp32 likelihoods: 1e-5), digits equal."""
    from sr.recognition.batch import ContinuousDecoder
    g = load_golden("G14_loop_grammar")
    Wg, ng = g["means"].shape[:2]
    hmms = [make_hmm(R, g["means"][i], g["vars"][i], g["w"][i], g["word_trans"]) for i in range(Wg)]
    U = int(g["n_utts"])
    for pen in (0, 1):
        pp = "p%d_" % pen
        dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=float(g[pp + "penalty"]), dtype=dtype, ctx=ctx)
        xs = [g[pp + "x%d" % u] for u in range(U)]
        on = dec.online(n_streams=U, max_frames=max(len(x) for x in xs))
        for t in range(0, max(len(x) for x in xs), chunk):
            on.push(np.arange(U), [x[t:t + chunk] for x in xs])
        words, info = on.result(want_path=True)
        ends = np.asarray(dec.lat.end_rows[0])
        rw = g[pp + "row_word"]
        for u in range(U):
            np.testing.assert_allclose(info["end_cost"][u], g[pp + "costs%d" % u][ends, -1], rtol=1e-10 if dtype == np.float64 else 1e-5)
            np.testing.assert_array_equal(info["paths"][u], g[pp + "path%d" % u])
            assert O.path_to_words(info["paths"][u], rw < 0, rw) == list(g[pp + "digits%d" % u]) == words[u]
        assert on.result()[0] == words
        on.close()


def test_online_capacity_and_form_errors(R, hip, ctx):
    """Through the real library: a push past max_frames, with an id twice or out of range, or with a column range outside
    an utterance is refused as a whole and changes nothing; K-layer, bigram and 17-word graphs are Unsupported."""
    from sr.recognition.batch import ContinuousDecoder
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    rng = np.random.default_rng(3)
    W, n, M, D = 4, 3, 2, 5
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    wt = [word_trans(rng, n) for _ in range(W)]
    hmms = [make_hmm(R, means[i], vars_[i], w[i], wt[i]) for i in range(W)]
    dec = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
    on = dec.online(n_streams=3, max_frames=12)
    xs = [rng.normal(size=(T, D)) * 2.0 for T in (9, 6, 4)]
    on.push([0, 1, 2], xs)
    before = on.result(want_path=True)
    b = hip.Batch(ctx, [rng.normal(size=(4, D)), rng.normal(size=(3, D))])
    b.loglik(dec.gmm, fetch=False)
    s = on.session                                                       # the binding itself: no Python-side checks
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
    for p, q in zip(after[1]["paths"], mid[1]["paths"]):
        np.testing.assert_array_equal(p, q)
    assert before[1]["frames"].tolist() == [9, 6, 4]
    with pytest.raises(ValueError):                                      # the same through the decoder: before the GPU is touched
        on.push([2, 0], [xs[2], xs[2]])
    with pytest.raises(hip.BackendError):
        s.result([3])
    s.push(b, [2, 1], first=[0, 1], count=[4, 2])                        # exactly to capacity is fine
    assert s.frames().tolist() == [12, 12, 8]
    on.close()
    b.close()
    # graph forms
    for graph in (packed_lattice(wt, n, [list(range(W))] * 3)[0],
                  packed_bigram_lattice(wt, n, rng.uniform(0.5, 3.0, size=(W, W)), None)[0],
                  packed_loop_lattice([wt[0]] * 17, n, 0.0)[0]):
        lat = hip.Lattices(ctx, [graph])
        with pytest.raises(hip.Unsupported):
            hip.OnlineSession(ctx, lat, 4, 10)
        lat.close()
    with pytest.raises(hip.Unsupported):
        ContinuousDecoder(hmms, n_layers=2, ctx=ctx).online(4, 10)
    lat = hip.Lattices(ctx, [packed_loop_lattice(wt, n, 0.0)[0]])
    lat.set_beam(3)
    with pytest.raises(hip.Unsupported):
        hip.OnlineSession(ctx, lat, 4, 10)
    lat.close()
