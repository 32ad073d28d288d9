# -*- coding: utf-8 -*-
"""Online isolated-word recognition on the device (gh_viterbi_chain_online.hip, gh_wordstream_*): the lane = chain sweep
carried across chunks, one cost column per stream.

The contract is "online == offline on the prefix, from two frames on":
  1. the dynamic program alone -- ONE resident likelihood matrix fed in random column ranges -- is BITWISE the one-shot
     sweep on the same matrix (`rec.costs(batch)`), for every lane mapping of the kernel, fp64 and fp32 likelihoods;
  2. a stream at exactly one frame shows the causal column 0 (tests/test_online_words_host.py: not the one-frame decode);
  3. end to end (frames in, 20-frame ticks, likelihoods per tick, shuffled ids, streams at different rates, resets and
     reused ids) it gives what `IsolatedWordRecognizer.recognize` gives on the whole utterances;
  4. at tick boundaries the running result is `recognize` of the prefix;
  5. the reference's own G3 decisions come out in chunks of 1, 7 and 50 frames;
  6. audio and recordings through the streaming front-end and endpointer equal the offline path;
  7. refusals through the real library change nothing, and every graph the session does not take is Unsupported."""
import numpy as np
import pytest

import stream_endpoints_ref as S
from conftest import load_golden
from online_ref import CarriedDecode

pytestmark = pytest.mark.gpu

TICK = 20


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


def word_trans(rng, n, skip=False):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.05, 0.6) if i < n - 1 else rng.uniform(0.0, 0.3)
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


def random_model(R, rng, W, n, skip, M=2, D=6):
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    hmms = [make_hmm(R, means[i], vars_[i], w[i], word_trans(rng, n, skip)) for i in range(W)]
    return hmms, means, vars_


# ------------------------------------------------------------------------------------------- 1: the DP yardstick
# (W, n, skip, M): the headline shape; a single one-state word; two-state words; skip arcs at a small width; 4 streams per wave
# with 12 idle lanes; exactly one stream per wave; two waves per stream, the second nearly empty; several waves per stream
# with skip arcs; 3 streams per wave with 1 idle lane; one-component mixtures (rec.costs takes the fused kernel there)
SHAPES = [(10, 5, False, 2), (1, 1, False, 2), (3, 2, False, 2), (7, 3, True, 2), (13, 8, True, 2), (64, 4, True, 2), (65, 3, False, 2),
          (100, 5, True, 2), (21, 7, False, 2), (10, 5, False, 1)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("W,n,skip,M", SHAPES)
def test_carried_sweep_is_bitwise_the_one_shot_sweep(R, hip, ctx, W, n, skip, M, dtype):
    """One whole-utterance batch with resident likelihoods, fed through push_batch(first, count) in random column ranges
    (0- and 1-frame ranges among them), against `rec.costs` on the same batch.  61 ragged utterances of >= 2 frames, some
    shorter than a word, on ids scattered over 67 streams."""
    from sr.recognition.batch import IsolatedWordRecognizer
    rng = np.random.default_rng(91 * W + n)
    D = 6
    hmms, means, vars_ = random_model(R, rng, W, n, skip, M=M, D=D)
    xs = []
    for u in range(61):
        if u % 9 == 0:
            xs.append(rng.normal(size=(int(rng.integers(2, max(3, n))), D)) * 2.0)      # shorter than a word (n >= 3)
            continue
        wd = int(rng.integers(0, W))
        Tw = int(rng.integers(max(2, n), 9 * n + 12))
        st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
        comp = rng.integers(0, M, size=Tw)
        xs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D)))
    rec = IsolatedWordRecognizer(hmms, dtype=dtype, ctx=ctx)
    assert rec.gmm.M == M and not rec.single
    b = hip.Batch(ctx, xs, dtype=dtype)
    T = np.asarray(b.lengths, dtype=np.int64)
    assert T.min() >= 2 and T.max() >= 17
    if M == 1:                                           # rec.costs would score inside the fused kernel: no [N, S] matrix
        b.loglik(rec.gmm, fetch=False)
        ref = rec.lat.viterbi(b, want_path=False)["end_cost_flat"].reshape(b.U, W)
    else:
        ref = rec.costs(b)                              # the one-shot sweep; the likelihood matrix stays resident
    on = rec.online(n_streams=67)
    ids = rng.permutation(67)[:b.U]
    pos = np.zeros(b.U, dtype=np.int64)
    while np.any(pos < T):
        cnt = np.minimum(rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 1000], size=b.U), T - pos)
        on.push_batch(ids, b, first=pos, count=cnt)
        pos += cnt
    np.testing.assert_array_equal(on.frames[ids], T)
    words, info = on.result(ids)
    assert np.isfinite(ref).any()
    np.testing.assert_array_equal(info["costs"], ref)
    np.testing.assert_array_equal(words, np.argmin(ref, axis=1))
    assert info["frames"].tolist() == T.tolist()
    untouched = np.setdiff1d(np.arange(67), ids)
    w0, i0 = on.result(untouched)
    assert w0.tolist() == [-1] * len(untouched) and np.all(np.isposinf(i0["costs"]))
    on.close()
    b.close()


# ------------------------------------------------------------------------------------------- 2: the one-frame rule
@pytest.mark.parametrize("W,n,skip", [(10, 5, False), (4, 1, False), (7, 3, True)])
def test_a_stream_of_one_frame_shows_the_causal_column(R, hip, ctx, W, n, skip):
    from sr.recognition.batch import IsolatedWordRecognizer
    rng = np.random.default_rng(5 + n)
    hmms, _, _ = random_model(R, rng, W, n, skip)
    rec = IsolatedWordRecognizer(hmms, ctx=ctx)
    xs = [rng.normal(size=(T, 6)) * 2.0 for T in (1, 4, 1)]
    b = hip.Batch(ctx, xs)
    nll = b.loglik(rec.gmm)                                                # [N, S], fetched
    on = rec.online(n_streams=4)
    on.push_batch([3, 0, 1], b, count=[1, 1, 1])
    words, info = on.result([3, 0, 1])
    off = np.concatenate([[0], np.cumsum(b.lengths)])
    for k in range(3):
        want = []
        for i, h in enumerate(hmms):
            cd = CarriedDecode(np.zeros(n, dtype=bool), h.transitions, [n - 1])
            cd.push(nll[off[k]:off[k] + 1, i * n:(i + 1) * n].T)
            want.append(cd.result()[0][0])
        want = np.array(want)
        np.testing.assert_array_equal(np.isinf(info["costs"][k]), np.isinf(want))
        assert np.all(np.isinf(want)) == (n > 1)
        fin = ~np.isinf(want)
        np.testing.assert_allclose(info["costs"][k][fin], want[fin], rtol=1e-12)
        assert words[k] == int(np.argmin(want))
    on.close()
    b.close()


# ------------------------------------------------------------------------------------------- 3, 4: configs[1], end to end
U_E2E = 400


@pytest.fixture(scope="module")
def c1(R):
    """The configs[1] model (10 words x 5 states x 8 mixtures, D = 39) and 400 one-word utterances of 60 .. 120 frames."""
    import bench
    wl = bench.synth_workload(1101, U_E2E, tmin=60, tmax=120)
    hmms = [make_hmm(R, wl["means"][i], wl["vars"][i], wl["w"][i], wl["trans"]) for i in range(wl["W"])]
    off = wl["off"]
    return dict(hmms=hmms, xs=[wl["X"][off[u]:off[u + 1]] for u in range(U_E2E)], words=wl["words"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_online_words_end_to_end_equal_recognize(hip, ctx, c1, dtype):
    """400 streams in 20-frame ticks through push(ids, chunks): shuffled id order, streams that sit ticks out and so
    progress at different rates, empty chunks, 30 streams reset half-way through ANOTHER utterance and their id reused.
    After the last tick: words == recognize(xs) on the whole utterances, costs 1e-12 (fp32 likelihoods: 1e-5).  An
    utterance whose two cheapest ONE-SHOT costs lie closer than 1e-9 relative (fp32: 1e-4) may be left out of the word
    comparison, at most 1 % of them; with this seed the one-shot costs leave out none."""
    from sr.recognition.batch import IsolatedWordRecognizer
    rng = np.random.default_rng(6)
    xs = c1["xs"]
    D = xs[0].shape[1]
    rec = IsolatedWordRecognizer(c1["hmms"], dtype=dtype, ctx=ctx)
    on = rec.online(n_streams=U_E2E)
    stream_of = rng.permutation(U_E2E)                                    # utterance u lives on stream stream_of[u]
    pos = np.zeros(U_E2E, dtype=np.int64)
    lens = np.array([len(x) for x in xs])
    decoy = {int(u): int(rng.integers(0, U_E2E)) for u in rng.choice(U_E2E, size=30, replace=False)}
    decoy_pos = {u: 0 for u in decoy}
    ticks = sat_out = empty = 0
    while np.any(pos < lens):
        live = np.flatnonzero(pos < lens)
        ids, chunks = [], []
        for u in rng.permutation(live):
            u = int(u)
            r = rng.random()
            if r < 0.15:
                sat_out += 1
                continue                                                  # not part of this tick's push
            if r < 0.25:
                empty += 1
                ids.append(stream_of[u]); chunks.append(np.zeros((0, D)))  # part of it with no frames
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
        assert ticks < 200
    assert not decoy and sat_out > 0 and empty > 0
    np.testing.assert_array_equal(on.frames[stream_of], lens)
    ref_words, ref_costs = rec.recognize(xs)
    words, info = on.result(stream_of)
    two = np.sort(ref_costs, axis=1)[:, :2]
    gap = (two[:, 1] - two[:, 0]) / two[:, 0]                             # from the one-shot costs alone
    keep = gap >= (1e-9 if dtype == np.float64 else 1e-4)
    print("smallest relative gap of the one-shot costs: %.3e; left out: %d" % (gap.min(), int(np.sum(~keep))))
    assert np.sum(~keep) <= U_E2E // 100
    np.testing.assert_array_equal(words[keep], ref_words[keep])
    np.testing.assert_allclose(info["costs"], ref_costs, rtol=1e-12 if dtype == np.float64 else 1e-5)
    assert np.mean(words == c1["words"]) > 0.9
    fw, fi = on.finish(stream_of)
    np.testing.assert_array_equal(fw, words)
    assert not on.frames.any()
    on.close()


def test_online_words_prefix_property(hip, ctx, c1):
    """16 streams, three tick boundaries each: result() == recognize of the frames pushed so far (words, costs)."""
    from sr.recognition.batch import IsolatedWordRecognizer
    xs = c1["xs"][:16]
    rec = IsolatedWordRecognizer(c1["hmms"], ctx=ctx)
    on = rec.online(n_streams=16)
    ids = np.arange(16)[::-1].copy()
    checked = 0
    for tick in range(1, 6):
        on.push(ids, [x[(tick - 1) * TICK:tick * TICK] for x in xs])
        if tick in (2, 3, 5):
            k = [min(tick * TICK, len(x)) for x in xs]
            ref_words, ref_costs = rec.recognize([x[:kk] for x, kk in zip(xs, k)])
            words, info = on.result(ids)
            np.testing.assert_array_equal(words, ref_words)
            np.testing.assert_allclose(info["costs"], ref_costs, rtol=1e-12)
            assert info["frames"].tolist() == k
            checked += 1
    assert checked == 3
    on.close()


# ------------------------------------------------------------------------------------------- 5: G3 in chunks
@pytest.mark.parametrize("chunk", [1, 7, 50])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", ["c2", "c1"])
def test_online_words_G3_in_chunks(R, hip, ctx, tag, dtype, chunk):
    """G3 (the reference's own HMM.evaluate values and decisions; c2: mixtures, c1: one-component mixtures), its utterances
    taken `chunk` frames at a time: final costs 1e-10 (fp32 likelihoods: 1e-3), words equal to the golden arg-min."""
    from sr.recognition.batch import IsolatedWordRecognizer
    g = load_golden("G3_isolated_decode_" + tag)
    W = g["means"].shape[0]
    hmms = [make_hmm(R, g["means"][i], g["vars"][i], g["w"][i], g["trans"]) for i in range(W)]
    U = len(g["words"])
    xs = [g["x%d" % u] for u in range(U)]
    rec = IsolatedWordRecognizer(hmms, dtype=dtype, ctx=ctx)
    assert rec.gmm.M == (1 if tag == "c1" else g["means"].shape[2]) and not rec.single
    on = rec.online(n_streams=U)
    for t in range(0, max(len(x) for x in xs), chunk):
        on.push(np.arange(U), [x[t:t + chunk] for x in xs])
    words, info = on.result()
    np.testing.assert_allclose(info["costs"], [g["evaluate_%d" % u] for u in range(U)], rtol=1e-10 if dtype == np.float64 else 1e-3)
    np.testing.assert_array_equal(words, g["words"])
    assert info["frames"].tolist() == [len(x) for x in xs]
    on.close()


# ------------------------------------------------------------------------------------------- 6: audio and recordings
A_TICK = 3200


@pytest.fixture(scope="module")
def audio(R, hip, ctx):
    """Eight 16 kHz recordings with two bursts each (the last one ends while speech is open), a 3-word model on the 39
    features of the front-end and the `feature_stats` normalisation of the recordings."""
    from sr.feature import feature_stats
    from sr.recognition.batch import IsolatedWordRecognizer
    rng = np.random.default_rng(19)
    rate = 16000
    lens = [42000, 43333, 45000, 46111, 48000, 44000, 47000, 36000]
    sigs = [S.burst_signal(rng, n, 40, [(4000, 10000), (24000, 30000)], freq=300.0 + 150 * i, rate=rate) for i, n in enumerate(lens)]
    sigs[7] = S.burst_signal(rng, lens[7], 40, [(4000, 10000), (24000, 36000)], rate=rate)       # ... or speech up to the end
    norm = feature_stats(sigs, rate)
    W, n, M, D = 3, 4, 2, 39
    trans = np.full((n, n), np.inf)
    for i in range(n):
        trans[i, i] = -np.log(0.8) if i < n - 1 else 0.0
        if i < n - 1:
            trans[i + 1, i] = -np.log(0.2)
    hmms = [make_hmm(R, rng.normal(size=(n, M, D)), rng.uniform(0.5, 1.5, size=(n, M, D)), rng.dirichlet(np.ones(M), size=n), trans)
            for _ in range(W)]
    return dict(sigs=sigs, norm=norm, rec=IsolatedWordRecognizer(hmms, ctx=ctx), rate=rate)


def ticks_of(sigs, lengths):
    """Ragged PCM chunks: stream k's t-th chunk has lengths[(k + t) % len(lengths)] samples."""
    pos = [0] * len(sigs)
    t = 0
    while any(p < len(s) for p, s in zip(pos, sigs)):
        live = [k for k, s in enumerate(sigs) if pos[k] < len(s)]
        chunks = []
        for k in live:
            c = lengths[(k + t) % len(lengths)]
            chunks.append(sigs[k][pos[k]:pos[k] + c])
            pos[k] += len(chunks[-1])
        yield live, chunks, [pos[k] >= len(sigs[k]) for k in live]
        t += 1


def test_push_audio_recognises_like_the_one_shot_path(hip, ctx, audio):
    from sr.feature import StreamingFrontend, features_from_signals
    rec, sigs, rate = audio["rec"], audio["sigs"], audio["rate"]
    b = features_from_signals(sigs, rate, normalize=audio["norm"])
    ref_costs = rec.costs(b)
    frames = b.lengths.tolist()
    b.close()
    fe = StreamingFrontend(8, rate, normalize=audio["norm"], max_chunk=A_TICK)
    on = rec.online(8, frontend=fe)
    for ids, chunks, end in ticks_of(sigs, [A_TICK, 777, 1600, 0, 2999, 161]):
        on.push_audio(ids, chunks, end)
    assert on.frames.tolist() == frames and fe.samples.tolist() == [len(s) for s in sigs]
    with pytest.raises(ValueError):
        on.push_audio([0], [sigs[0][:A_TICK]])                              # the utterance has ended
    words, info = on.result(np.arange(8))
    np.testing.assert_array_equal(words, np.argmin(ref_costs, axis=1))
    np.testing.assert_allclose(info["costs"], ref_costs, rtol=1e-12)
    on.finish([2])                                                          # frees the id in the front-end too
    assert fe.samples[2] == 0 and on.frames[2] == 0
    for ids, chunks, end in ticks_of([sigs[0]], [A_TICK]):
        on.push_audio([2], chunks, end)
    words2, info2 = on.result([2])
    assert words2[0] == words[0]
    np.testing.assert_allclose(info2["costs"][0], info["costs"][0], rtol=1e-12)
    on.close()
    fe.close()


def test_push_recording_recognises_like_the_offline_path(hip, ctx, audio):
    import sr.audio_capture as AC
    from sr.feature import StreamingFrontend, features_from_signals
    rec, sigs, rate = audio["rec"], audio["sigs"], audio["rate"]
    cfg = AC.default_config(rate)
    det = AC.detect_endpoints(sigs, dict(cfg), max_segments=8)
    assert det["n_segments"].tolist() == [2] * 8 and det["open"].tolist() == [False] * 7 + [True]
    begin, stop = AC.trim_ranges(det, [len(x) for x in sigs], dict(cfg))
    which = np.repeat(np.arange(8), det["n_segments"])
    b = features_from_signals([sigs[r][s:e] for r, s, e in zip(which, begin, stop)], rate, normalize=audio["norm"])
    assert min(b.lengths) >= 2
    ref_costs = rec.costs(b)
    b.close()
    offline = [[] for _ in sigs]
    for j, (r, s, e) in enumerate(zip(which, begin, stop)):
        offline[r].append((int(s), int(e), bool(det["open"][r]) and len(offline[r]) == 1, int(np.argmin(ref_costs[j])), ref_costs[j]))
    ep = AC.StreamingEndpointer(8, AC.default_config(rate), max_chunk=A_TICK)
    fe = StreamingFrontend(8, rate, normalize=audio["norm"], max_chunk=ep.max_piece)
    with pytest.raises(ValueError):
        rec.online(8, frontend=StreamingFrontend(8, rate, normalize=audio["norm"], max_chunk=A_TICK), endpointer=ep)
    on = rec.online(8, frontend=fe, endpointer=ep)
    got = [[] for _ in sigs]
    for ids, chunks, end in ticks_of(sigs, [A_TICK, 777, 1600, 0, 2999, 161]):
        for u in on.push_recording(ids, chunks, end):
            got[u["stream"]].append(u)
    for r, per in enumerate(offline):
        assert [(u["begin"], u["stop"], u["open"]) for u in got[r]] == [(s, e, o) for s, e, o, _, _ in per], r
        assert [u["word"] for u in got[r]] == [w for _, _, _, w, _ in per], r
        for u, (_, _, _, _, want) in zip(got[r], per):
            np.testing.assert_allclose(u["costs"], want, rtol=1e-12)
    assert on.frames.tolist() == [0] * 8 and fe.samples.tolist() == [0] * 8 and ep.samples.tolist() == [len(s) for s in sigs]
    on.close()
    fe.close()
    ep.close()


# ------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_through_the_real_library(R, hip, ctx):
    """A push with an id twice, an id out of range or a column range outside the utterance is refused as a whole and
    changes nothing; loop, bigram and K-layer graphs, chains of unequal length, 12-state chains, a beam and a
    single-Gaussian recogniser are Unsupported; a reset id decodes a fresh utterance."""
    from sr.recognition.batch import IsolatedWordRecognizer
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    rng = np.random.default_rng(3)
    W, n, D = 4, 3, 6
    hmms, _, _ = random_model(R, rng, W, n, False)
    wt = [h.transitions for h in hmms]
    rec = IsolatedWordRecognizer(hmms, ctx=ctx)
    on = rec.online(n_streams=3)
    xs = [rng.normal(size=(T, D)) * 2.0 for T in (9, 6, 4)]
    on.push([0, 1, 2], xs)
    b = hip.Batch(ctx, [rng.normal(size=(4, D)), rng.normal(size=(3, D))])
    s = on.session                                                       # the binding itself: no Python-side checks
    with pytest.raises(hip.BackendError):
        s.push(b, [1, 0])                                                # a batch without likelihoods
    b.loglik(rec.gmm, fetch=False)
    mid = s.result()
    assert s.frames().tolist() == [9, 6, 4] == on.frames.tolist()
    for ids, kw in (([2, 2], {}), ([2, 3], {}), ([-1, 2], {}),           # an id twice, ids out of range
                    ([2, 1], dict(first=[2, 0], count=[3, 1])),          # columns [2, 5) of a 4-frame utterance
                    ([2, 1], dict(first=[0, -1])), ([2, 1], dict(count=[4, 4]))):
        with pytest.raises(hip.BackendError):
            s.push(b, ids, **kw)
        assert s.frames().tolist() == [9, 6, 4]
    after = s.result()
    np.testing.assert_array_equal(after["costs"], mid["costs"])
    np.testing.assert_array_equal(after["best"], mid["best"])
    with pytest.raises(ValueError):                                      # the same through the recogniser: before the GPU is touched
        on.push([2, 2], [xs[2], xs[2]])
    with pytest.raises(hip.BackendError):
        s.result([3])
    with pytest.raises(hip.BackendError):
        s.reset([3])
    # reset, then reuse of an id: a fresh utterance
    on.reset([1])
    assert on.frames.tolist() == [9, 0, 4] and s.frames().tolist() == [9, 0, 4]
    on.push([1], [xs[0][:5]])
    on.push([1], [xs[0][5:]])
    words, info = on.result([1, 0])
    ref_words, ref_costs = rec.recognize([xs[0]])
    assert words.tolist() == [int(ref_words[0])] * 2
    np.testing.assert_allclose(info["costs"], np.repeat(ref_costs, 2, axis=0), rtol=1e-12)
    on.close()
    b.close()
    # graph forms
    def stacked(trans_list, states=None):
        sizes = [len(t) for t in trans_list]
        o = np.concatenate([[0], np.cumsum(sizes)])
        to, frm, cost = [], [], []
        for i, t in enumerate(trans_list):
            a, c = np.nonzero(~np.isinf(t))
            to.append(a + o[i]); frm.append(c + o[i]); cost.append(t[a, c])
        return dict(row_state=np.arange(o[-1], dtype=np.int32) if states is None else states, arc_to=np.concatenate(to),
                    arc_from=np.concatenate(frm), arc_cost=np.concatenate(cost), start_rows=o[:-1], end_rows=o[1:] - 1)
    for graph in (packed_loop_lattice(wt, n, 0.0)[0],
                  packed_bigram_lattice(wt, n, rng.uniform(0.5, 3.0, size=(W, W)), None)[0],
                  packed_lattice(wt, n, [list(range(W))] * 3)[0],
                  stacked([word_trans(rng, 3), word_trans(rng, 4), word_trans(rng, 3)]),          # chains of unequal length
                  stacked([word_trans(rng, 12)] * 2)):                                             # n = 12
        lat = hip.Lattices(ctx, [graph])
        with pytest.raises(hip.Unsupported):
            hip.WordStreamSession(ctx, lat, 4)
        lat.close()
    lat = hip.Lattices(ctx, [stacked(wt)])
    hip.WordStreamSession(ctx, lat, 4).close()                           # (the same graph without a beam is taken)
    lat.set_beam(3)
    with pytest.raises(hip.Unsupported):
        hip.WordStreamSession(ctx, lat, 4)
    lat.close()
    single = []
    for h in hmms:
        m = R.HMM(n)
        m.mu, m.sigma, m.transitions = h.mu.copy(), h.sigma.copy(), h.transitions.copy()
        m.use_gmm, m.gmm_states = False, None
        single.append(m)
    with pytest.raises(hip.Unsupported):
        IsolatedWordRecognizer(single, ctx=ctx).online(4)
