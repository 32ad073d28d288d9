# -*- coding: utf-8 -*-
"""Online decoding on the K-layer word lattice on the device (gh_viterbi_layers_online.hip, gh_online_create_layers): the
layer-form sweep carried across chunks, one wave per stream, lane = (layer mod 4, word), two register sets.

The contract is "online == offline on the prefix", from two frames on:
  1. the dynamic program alone -- ONE resident likelihood matrix fed in random column ranges -- is BITWISE the one-shot
     layer kernel on the same matrix (end costs array_equal, chosen ends, paths, labels), for every instantiated N x skip;
  2. chunks of 1 to 9 frames with a result after every push (a left-aligned partial word in the history is overwritten
     by the next push); a ONE-frame stream reports the causal column 0;
  3. predecessor ties (`cand == rm` in several lanes, also across the readlane from layer 3 into layer 4), all-inf
     candidates, reused ids, streams that sit a tick out;
  4. the reference's own G4 decodes in chunks of 1, 7 and 50 frames;
  5. end to end (frames in, 20-frame ticks, likelihoods per tick) against `ContinuousDecoder.decode_batch` of the prefix,
     with word times, and from audio;
  6. refusals through the real library."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import ref_numpy as O
from online_ref import CarriedDecode
from test_gpu_online import c5, make_hmm, word_trans, TICK  # noqa: F401  (c5: the fixture of the configs[4] recipe)

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


def make_decoder(R, ctx, rng, W, n, K, skip, M=2, D=6, dtype=np.float64, twins=False):
    """(a K-layer decoder over W random word models, their means, variances and transitions); twins: words 2 i and
    2 i + 1 are the same model (states and transitions)."""
    from sr.recognition.batch import ContinuousDecoder
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    wt = [word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)]
    if twins:
        for i in range(1, W, 2):
            means[i], vars_[i], w[i], wt[i] = means[i - 1], vars_[i - 1], w[i - 1], wt[i - 1]
    hmms = [make_hmm(R, means[i], vars_[i], w[i], wt[i]) for i in range(W)]
    return ContinuousDecoder(hmms, n_layers=K, dtype=dtype, ctx=ctx), means, vars_, wt


def make_utts(rng, means, vars_, K, U, n_short):
    """U utterances of K words; the first n_short of them are too short for K words (unreachable ends)."""
    W, n, M, D = means.shape
    xs = []
    for u in range(U):
        if u < n_short:
            xs.append(rng.normal(size=(int(rng.integers(2, K * (n - 1) + 2)), D)) * 2.0)
            continue
        segs = []
        for wd in rng.integers(0, W, size=K):
            Tw = int(rng.integers(n, 3 * n + 4))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            comp = rng.integers(0, M, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D)))
        xs.append(np.concatenate(segs))
    return xs


def row_word_of(dec):
    return np.where(dec.row_state >= 0, dec.row_state // dec.n, -1).astype(np.int32)


def assert_bitwise_the_one_shot_decode(dec, on, ids, b, K):
    """Streams `ids` hold the utterances of `b` (same resident matrix): everything equals the one-shot layer decode."""
    ref = dec.lat.viterbi(b, want_path=True)
    words, info = on.result(ids, want_path=True)
    np.testing.assert_array_equal(info["end_cost"].reshape(-1), ref["end_cost_flat"])
    np.testing.assert_array_equal(info["best_end"], ref["best_end"])
    for u in range(b.U):
        np.testing.assert_array_equal(info["paths"][u], ref["paths"][u])
    lab = dec.lat.viterbi_labels(b, row_word_of(dec), max_labels=K + 1)
    words2, info2 = on.result(ids)
    assert words2 == [[int(v) for v in l] for l in lab["labels"]] == words
    np.testing.assert_array_equal(info2["end_cost"].reshape(-1), ref["end_cost_flat"])
    np.testing.assert_array_equal(info2["best_end"], ref["best_end"])
    return ref, words


def one_frame_column(hip, dec, wt, K, x1):
    """(end costs, chosen end) of `CarriedDecode` after the one frame x1 [1, D], on the device's own likelihoods."""
    from sr.recognition.continuous_speech import packed_lattice
    b = hip.Batch(dec.ctx, [x1])
    nll = np.asarray(b.loglik(dec.gmm, fetch=True), dtype=np.float64)
    b.close()
    g = packed_lattice(wt, dec.n, [list(range(len(wt)))] * K)[0]
    np.testing.assert_array_equal(g["row_state"], dec.row_state)
    Rr = len(dec.row_state)
    trans = np.full((Rr, Rr), np.inf)
    trans[g["arc_to"], g["arc_from"]] = g["arc_cost"]
    nes = dec.row_state < 0
    cd = CarriedDecode(nes, trans, g["end_rows"])
    cd.push(np.where(nes[:, None], 0.0, nll[:, np.maximum(dec.row_state, 0)].T))
    ec, bi, path = cd.result()
    assert len(path) == 0
    return ec, bi


# every instantiated N x skip, CPW from 5 down to 1, one register set partly filled (K < 4), exactly full (K = 4), the carry
# from layer 3 into layer 4 (K = 5), both sets full (K = 8)
SHAPES = [(10, 5, 7, False), (11, 5, 7, False), (1, 2, 1, False), (3, 2, 8, False), (16, 3, 4, True), (5, 8, 5, True),
          (7, 4, 3, False), (10, 5, 2, True), (4, 6, 6, False), (2, 7, 8, True), (3, 4, 2, True), (2, 6, 3, True)]


@pytest.mark.parametrize("W,n,K,skip", SHAPES)
def test_online_layers_sweep_is_bitwise_the_layer_kernel(R, hip, ctx, W, n, K, skip):
    """The DP yardstick: one whole-utterance batch with resident likelihoods, fed through push_batch(first, count) in
    random column ranges (0- and 1-frame ranges among them, ranges that end inside a decision word), against
    lat.viterbi and viterbi_labels on the same batch.  61 ragged utterances, 12 of them too short for K words; ids
    scattered over 67 streams."""
    rng = np.random.default_rng(91 * W + 7 * n + K)
    dec, means, vars_, _ = make_decoder(R, ctx, rng, W, n, K, skip)
    assert "layers" in dec.lat.forms()
    xs = make_utts(rng, means, vars_, K, 61, 12)
    for dtype in (np.float64, np.float32):
        b = hip.Batch(ctx, xs, dtype=dtype)
        T = np.asarray(b.lengths, dtype=np.int64)
        on = dec.online_layers(n_streams=67, max_frames=int(T.max()))
        assert isinstance(on.session, hip.OnlineLayersSession)
        ids = rng.permutation(67)[:b.U]
        pos = np.zeros(b.U, dtype=np.int64)
        while np.any(pos < T):
            cnt = np.minimum(rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 1000], size=b.U), T - pos)
            on.push_batch(ids, b, first=pos, count=cnt)                 # (the first call computes the likelihoods, once)
            pos += cnt
        np.testing.assert_array_equal(on.frames[ids], T)
        ref, _ = assert_bitwise_the_one_shot_decode(dec, on, ids, b, K)
        assert np.isfinite(ref["end_cost_flat"]).any()
        if K * (n - 1) >= 4:
            assert np.isinf(ref["end_cost_flat"]).any()               # the short utterances cannot hold K words
        on.close()
        b.close()


@pytest.mark.parametrize("chunk", [1, 2, 3, 4, 5, 6, 7, 8, 9])
@pytest.mark.parametrize("W,n,K,skip", [(10, 5, 7, False), (5, 8, 5, True)])
def test_online_layers_result_after_every_push(R, hip, ctx, W, n, K, skip, chunk):
    """`chunk` frames at a time with a result after EVERY push: a chunk that ends inside a decision word leaves it left
    aligned in the history, and the next push overwrites it.  From two frames on: words, chosen end, paths and begins
    equal decode_batch of the prefix, end costs to 1e-12 (the likelihoods of the prefix batch are computed separately:
    the tolerance of test_online_end_to_end_equals_decode_batch); a one-frame stream gives the pinned column 0."""
    rng = np.random.default_rng(500 + 10 * n + chunk)
    dec, means, vars_, wt = make_decoder(R, ctx, rng, W, n, K, skip)
    xs = [x[:2 * K * n] for x in make_utts(rng, means, vars_, K, 5, 1)]   # (short enough for a result after every push)
    Tmax = max(len(x) for x in xs)
    on = dec.online_layers(n_streams=8, max_frames=Tmax, times=True)
    ids = np.array([6, 0, 3, 7, 2])
    checked = full = 0
    for t in range(0, Tmax, chunk):
        on.push(ids, [x[t:t + chunk] for x in xs])
        pos = [min(len(x), t + chunk) for x in xs]
        words, info = on.result(ids)
        wp, ip = on.result(ids, want_path=True)
        assert info["frames"].tolist() == pos and words == wp
        if t + chunk == 1:
            for u in range(len(xs)):
                ec, bi = one_frame_column(hip, dec, wt, K, xs[u][:1])
                np.testing.assert_array_equal(info["end_cost"][u], ec)    # (every end is +inf after one frame)
                assert info["best_end"][u] == bi == ip["best_end"][u] == W - 1
                assert words[u] == [] and len(ip["paths"][u]) == 0 and len(info["begins"][u]) == 0
            continue
        b = hip.Batch(ctx, [x[:p] for x, p in zip(xs, pos)])
        ref_words, ref = dec.decode_batch(b, want_path=True, want_times=True)
        assert words == ref_words
        np.testing.assert_array_equal(info["best_end"], ref["best_end"])
        np.testing.assert_allclose(info["end_cost"].reshape(-1), ref["end_cost_flat"], rtol=1e-12)
        for u in range(len(xs)):
            np.testing.assert_array_equal(ip["paths"][u], ref["paths"][u])
            np.testing.assert_array_equal(info["begins"][u], ref["begins"][u])
            np.testing.assert_array_equal(ip["begins"][u], ref["begins"][u])
        b.close()
        checked += 1
        full += sum(len(wd) == K for wd in words)
    assert checked >= 2 and full >= 1
    on.close()


def test_online_layers_predecessor_ties(R, hip, ctx):
    """Words 2 i and 2 i + 1 are the same model, so their costs are equal bit for bit in every layer and `cand == rm` holds
    in (at least) two lanes of every row minimum, the one whose minimum crosses from layer 3 into layer 4 included.  One
    frame at a time on one resident matrix: paths and labels are the one-shot decode's, and the lower word of a pair wins."""
    W, n, K = 6, 3, 6
    rng = np.random.default_rng(77)
    dec, means, vars_, _ = make_decoder(R, ctx, rng, W, n, K, False, twins=True)
    xs = make_utts(rng, means, vars_, K, 9, 2)
    b = hip.Batch(ctx, xs)
    nll = np.asarray(b.loglik(dec.gmm, fetch=True))
    for i in range(1, W, 2):                                              # the twins' likelihoods are equal bit for bit
        np.testing.assert_array_equal(nll[:, i * n:(i + 1) * n], nll[:, (i - 1) * n:i * n])
    T = np.asarray(b.lengths, dtype=np.int64)
    on = dec.online_layers(n_streams=9, max_frames=int(T.max()))
    ids = np.arange(9)[::-1].copy()
    for t in range(int(T.max())):
        on.push_batch(ids, b, first=np.minimum(t, T), count=(t < T).astype(np.int64))
    ref, words = assert_bitwise_the_one_shot_decode(dec, on, ids, b, K)
    whole = [wd for wd in words if len(wd) == K]
    # K words each, every layer boundary tied: the first minimum of a row (the lower twin) wins inside the lattice, the LAST of
    # equal end points (the upper twin) at its end
    assert len(whole) >= 5 and all(v % 2 == 0 for wd in whole for v in wd[:-1]) and all(wd[-1] % 2 == 1 for wd in whole)
    P = W * n
    crossed = sum(bool(np.any(p[:, 0] == 4 * (P + 1))) for p in ref["paths"])      # the non-emitting row in front of layer 4
    assert crossed >= 5
    on.close()
    b.close()


def test_online_layers_all_inf_candidates(R, hip, ctx):
    """Utterances too short for K words, in three pushes: every end cost is +inf, every candidate of the end selection and of
    the back-trace ties at +inf; the chosen end, the path the walk takes through the +inf cells (it follows the first existing
    arc and ends in column 0) and the labels on it are the one-shot decode's."""
    W, n, K = 4, 5, 7
    rng = np.random.default_rng(78)
    dec, means, vars_, _ = make_decoder(R, ctx, rng, W, n, K, False)
    xs = [rng.normal(size=(T, 6)) * 2.0 for T in (2, 3, 7, 12, 20, K * (n - 1))]  # (K words need K (n - 1) + 1 frames)
    b = hip.Batch(ctx, xs)
    T = np.asarray(b.lengths, dtype=np.int64)
    on = dec.online_layers(n_streams=6, max_frames=int(T.max()))
    ids = np.array([4, 1, 5, 0, 2, 3])
    cuts = [np.zeros(6, dtype=np.int64), T // 3, T - 1, T]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        on.push_batch(ids, b, first=lo, count=hi - lo)
    ref, words = assert_bitwise_the_one_shot_decode(dec, on, ids, b, K)
    assert np.all(np.isinf(ref["end_cost_flat"])) and ref["best_end"].tolist() == [W - 1] * 6
    assert all(1 <= len(wd) <= K for wd in words)                         # (the words the walk through the +inf cells passes)
    on.close()
    b.close()


def test_online_layers_ids_reuse_sitting_out_and_reset(R, hip, ctx):
    """A stream id reused after `finish` equals a fresh session; a stream that sits a tick out (count 0, or not named)
    keeps its state; reset(None) frees every stream."""
    W, n, K = 5, 4, 5
    rng = np.random.default_rng(79)
    dec, means, vars_, _ = make_decoder(R, ctx, rng, W, n, K, True)
    xs = make_utts(rng, means, vars_, K, 6, 1)
    b = hip.Batch(ctx, xs)
    T = np.asarray(b.lengths, dtype=np.int64)
    on = dec.online_layers(n_streams=6, max_frames=int(T.max()))
    # first life of the ids: the utterances in REVERSED assignment, half-way and to the end, then finish / reset
    rev = np.arange(6)[::-1].copy()
    on.push_batch(rev, b, count=T // 2)
    on.push_batch(rev, b, first=T // 2)
    assert_bitwise_the_one_shot_decode(dec, on, rev, b, K)
    on.finish(rev[:3])
    assert on.frames[rev[:3]].tolist() == [0, 0, 0] and np.all(on.frames[rev[3:]] == T[3:])
    on.reset()
    assert not on.frames.any() and on.result()[1]["best_end"].tolist() == [-1] * 6
    # second life: stream u takes utterance u, three frames a tick; odd streams sit every other tick out (count 0), stream 0
    # every third
    ids = np.arange(6)
    pos = np.zeros(6, dtype=np.int64)
    tick = 0
    while np.any(pos < T):
        cnt = np.minimum(3, T - pos)
        if tick % 2:
            cnt[1::2] = 0
        if tick % 3 == 0:
            cnt[0] = 0
        before = on.frames
        on.push_batch(ids, b, first=pos, count=cnt)
        np.testing.assert_array_equal(on.frames, before + cnt)
        pos += cnt
        tick += 1
    assert_bitwise_the_one_shot_decode(dec, on, ids, b, K)
    fresh = dec.online_layers(n_streams=6, max_frames=int(T.max()))
    fresh.push_batch(ids, b)
    a, c = on.result(ids, want_path=True), fresh.result(ids, want_path=True)
    assert a[0] == c[0]
    np.testing.assert_array_equal(a[1]["end_cost"], c[1]["end_cost"])
    np.testing.assert_array_equal(a[1]["best_end"], c[1]["best_end"])
    for p, q in zip(a[1]["paths"], c[1]["paths"]):
        np.testing.assert_array_equal(p, q)
    on.close()
    fresh.close()
    b.close()


@pytest.mark.parametrize("chunk", [1, 7, 50])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_layers_G4_in_chunks(R, hip, ctx, dtype, chunk):
    """G4 (the reference's own decode of the K = 1, 2, 3, 7 lattices), its utterance taken `chunk` frames at a time: paths
    BIT-EXACT to the golden, end costs 1e-10 (fp32 likelihoods: 1e-5), digits equal."""
    from sr.recognition.batch import ContinuousDecoder
    g = load_golden("G4_lattice_decode")
    Wg = g["means"].shape[0]
    hmms = [make_hmm(R, g["means"][i], g["vars"][i], g["w"][i], g["word_trans"]) for i in range(Wg)]
    for K in (1, 2, 3, 7):
        p = "K%d_" % K
        dec = ContinuousDecoder(hmms, n_layers=K, dtype=dtype, ctx=ctx)
        np.testing.assert_array_equal(dec.lat.end_rows[0], g[p + "ends"])
        x = g[p + "x"]
        on = dec.online_layers(n_streams=2, max_frames=len(x))
        for t in range(0, len(x), chunk):
            on.push([1], [x[t:t + chunk]])
        words, info = on.result([1], want_path=True)
        rw = g[p + "row_word"]
        np.testing.assert_allclose(info["end_cost"][0], g[p + "costs"][np.asarray(g[p + "ends"]), -1],
                                   rtol=1e-10 if dtype == np.float64 else 1e-5)
        np.testing.assert_array_equal(info["paths"][0], g[p + "path"])
        assert O.path_to_words(info["paths"][0], rw < 0, rw) == list(g[p + "digits"]) == words[0]
        assert on.result([1])[0] == words
        on.close()


U_E2E = 100


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_online_layers_end_to_end_equals_decode_batch_of_the_prefix(hip, ctx, c5, dtype):
    """100 seven-word utterances of the configs[4] recipe in 20-frame ticks through push(ids, chunks): shuffled ids, streams
    that sit ticks out and so progress at different rates.  At every fourth tick words, chosen ends and begins equal
    decode_batch(prefix, want_times=True), end costs to 1e-12 (fp32 likelihoods: 1e-5; likelihoods computed per tick); after
    the last tick `finish` equals decode_batch of the whole utterances, paths included."""
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(6)
    xs = c5["xs"][:U_E2E]
    L = np.array([len(x) for x in xs])
    dec = ContinuousDecoder(c5["hmms"], n_layers=7, dtype=dtype, ctx=ctx)
    assert "layers" in dec.lat.forms()
    on = dec.online_layers(n_streams=U_E2E + 5, max_frames=int(L.max()), times=True)
    stream_of = rng.permutation(U_E2E + 5)[:U_E2E]                        # utterance u lives on stream stream_of[u]
    pos = np.zeros(U_E2E, dtype=np.int64)
    rtol = 1e-12 if dtype == np.float64 else 1e-5
    ticks = checked = 0
    while np.any(pos < L):
        live = np.flatnonzero(pos < L)
        order = rng.permutation(live)
        order = order[rng.random(len(order)) >= 0.2]                      # a fifth of the streams sits the tick out
        on.push(stream_of[order], [xs[u][pos[u]:pos[u] + TICK] for u in order])
        pos[order] = np.minimum(pos[order] + TICK, L[order])
        ticks += 1
        assert ticks < 100
        if ticks % 4 == 0:
            some = np.flatnonzero(pos >= 2)
            b = hip.Batch(ctx, [xs[u][:pos[u]] for u in some], dtype=dtype)
            ref_words, ref = dec.decode_batch(b, want_times=True)
            words, info = on.result(stream_of[some])
            assert words == ref_words and info["frames"].tolist() == pos[some].tolist()
            np.testing.assert_array_equal(info["best_end"], ref["best_end"])
            for x, y in zip(info["begins"], ref["begins"]):
                np.testing.assert_array_equal(x, y)
            np.testing.assert_allclose(info["end_cost"].reshape(-1), ref["end_cost_flat"], rtol=rtol)
            b.close()
            checked += 1
    assert checked >= 3 and len(set(pos.tolist())) > 1
    np.testing.assert_array_equal(on.frames[stream_of], L)
    b = hip.Batch(ctx, xs, dtype=dtype)
    ref_words, ref = dec.decode_batch(b, want_path=True, want_times=True)
    words, info = on.result(stream_of, want_path=True)
    assert words == ref_words
    for p, q in zip(info["paths"], ref["paths"]):
        np.testing.assert_array_equal(p, q)
    fin, fi = on.finish(stream_of)
    assert fin == ref_words == dec.decode_batch(b)[0] and not on.frames.any()
    np.testing.assert_array_equal(fi["best_end"], ref["best_end"])
    for x, y in zip(fi["begins"], ref["begins"]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_allclose(fi["end_cost"].reshape(-1), ref["end_cost_flat"], rtol=rtol)
    truth = [list(map(int, w)) for w in c5["words"][:U_E2E]]
    assert np.mean([a == t for a, t in zip(words, truth)]) > 0.9
    b.close()
    on.close()


def test_online_layers_push_audio_decodes_like_the_one_shot_path(R, hip, ctx):
    """A small K-layer decoder of 39 dimensions behind a StreamingFrontend, int16 audio in uneven chunks: the final words
    (and begins) equal decode_batch on features_from_signals(..., normalize=) of the whole signals."""
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    from test_gpu_audio_capture import burst_signal
    rng = np.random.default_rng(18)
    dec, _, _, _ = make_decoder(R, ctx, rng, 6, 3, 4, False, D=39)
    rate, chunk = 16000, 3200
    sigs = [burst_signal(rng, k, 40, [(k // 4, k // 2), (5 * k // 8, 7 * k // 8)], freq=300.0 + 150 * i, rate=rate)
            for i, k in enumerate([8000, 11111, 14000])]
    norm = feature_stats(sigs, rate)
    b = features_from_signals(sigs, rate, normalize=norm)
    ref_words, ref = dec.decode_batch(b, want_times=True)
    frames = b.lengths.tolist()
    fe = StreamingFrontend(3, rate, normalize=norm, max_chunk=chunk)
    on = dec.online_layers(3, max_frames=max(frames), frontend=fe, times=True)
    assert isinstance(on.session, hip.OnlineLayersSession)
    pos = [0, 0, 0]
    while any(p < len(s) for p, s in zip(pos, sigs)):                     # uneven chunks, streams at different rates
        live = [k for k in range(3) if pos[k] < len(sigs[k])]
        cnt = [int(rng.choice([0, 1, 160, 401, 1777, chunk])) for _ in live]
        on.push_audio(live, [sigs[k][pos[k]:pos[k] + c] for k, c in zip(live, cnt)], [pos[k] + c >= len(sigs[k]) for k, c in zip(live, cnt)])
        for k, c in zip(live, cnt):
            pos[k] = min(pos[k] + c, len(sigs[k]))
    assert on.frames.tolist() == frames and fe.samples.tolist() == [len(s) for s in sigs]
    words, info = on.result(np.arange(3))
    assert words == ref_words and all(len(wd) == 4 for wd in words)
    np.testing.assert_array_equal(info["best_end"], ref["best_end"])
    for x, y in zip(info["begins"], ref["begins"]):
        np.testing.assert_array_equal(x, y)
    on.finish([1])                                                        # frees the id in the front-end too
    assert fe.samples[1] == 0 and on.frames[1] == 0
    b.close(); on.close(); fe.close()


def test_online_layers_refusals(R, hip, ctx):
    """Through the real library: the graphs gh_online_create_layers does not take, each refused by name before anything
    is allocated; commit / tail; a push past max_frames moves no stream; online() still refuses the layers decoder."""
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    rng = np.random.default_rng(41)
    n = 3
    wt = [word_trans(rng, n) for _ in range(17)]
    wt2, wt12 = [word_trans(rng, 2) for _ in range(2)], [word_trans(rng, 12) for _ in range(2)]
    huge = 0x7fffffff                                                     # streams no device holds: refused before it is asked
    for graphs, word in (([packed_loop_lattice(wt[:4], n, 0.0)[0]], "word-loop graph"),
                         ([packed_bigram_lattice(wt[:4], n, rng.uniform(0.5, 3.0, size=(4, 4)), None)[0]], "bigram grammar"),
                         ([packed_lattice(wt, n, [list(range(17))] * 3)[0]], "more than 16 words"),
                         ([packed_lattice(wt2, 2, [[0, 1]] * 9)[0]], "more than 8 layers"),
                         ([packed_lattice(wt12, 12, [[0, 1]] * 2)[0]], "more than 8 states"),
                         ([packed_lattice(wt[:4], n, [list(range(4))] * 2)[0], packed_lattice(wt[:4], n, [list(range(4))] * 3)[0]],
                          "several graphs")):
        lat = hip.Lattices(ctx, graphs)
        with pytest.raises(hip.Unsupported, match=word):
            hip.OnlineLayersSession(ctx, lat, 4, 10)
        with pytest.raises(hip.Unsupported, match=word):                  # the graph is judged before the size
            hip.OnlineLayersSession(ctx, lat, huge, 10)
        lat.close()
    beam = hip.Lattices(ctx, [packed_lattice(wt[:4], n, [list(range(4))] * 3)[0]])
    beam.set_beam(3)
    with pytest.raises(hip.Unsupported, match="beam"):
        hip.OnlineLayersSession(ctx, beam, 4, 10)
    beam.close()
    # the other entry points go on refusing a K-layer lattice, and name the one that takes it
    layers = hip.Lattices(ctx, [packed_lattice(wt[:4], n, [list(range(4))] * 3)[0]])
    for cls in (hip.OnlineSession, hip.OnlineBigramSession, hip.OnlineWideSession, hip.OnlineBigramWideSession):
        with pytest.raises(hip.Unsupported, match="K-layer.*gh_online_create_layers takes it"):
            cls(ctx, layers, 4, 10)
    layers.close()
    dec, _, _, _ = make_decoder(R, ctx, rng, 4, n, 3, False, D=5)
    with pytest.raises(hip.Unsupported, match="online_layers takes it"):
        dec.online(4, 10)
    with pytest.raises(hip.Unsupported, match="online_layers takes it"):
        dec.online_bigram(4, 10)
    # a layer session does not settle
    on = dec.online_layers(n_streams=3, max_frames=12, times=True)
    s = on.session
    xs = [rng.normal(size=(T, 5)) * 2.0 for T in (9, 6, 4)]
    on.push([0, 1, 2], xs)
    for call in (s.commit, s.tail):
        with pytest.raises(hip.Unsupported, match="does not settle"):
            call()
        with pytest.raises(hip.Unsupported, match="does not settle"):
            call([0])
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(hip.Unsupported):
            call([0])
    # a push past max_frames: refused as a whole, by the decoder before the GPU is touched and by the library itself
    mid = on.result(want_path=True)
    with pytest.raises(ValueError):
        on.push([2, 0], [xs[2], xs[2]])                                   # stream 0: 9 + 4 > 12 -- stream 2 must not move either
    assert on.frames.tolist() == [9, 6, 4] == s.frames().tolist()
    b = hip.Batch(ctx, [xs[2], xs[2]])
    b.loglik(dec.gmm, fetch=False)
    for ids, kw in (([2, 0], {}), ([2, 2], {}), ([2, 3], {}), ([2, 1], dict(first=[2, 0], count=[3, 1]))):
        with pytest.raises(hip.BackendError):
            s.push(b, ids, **kw)
        assert s.frames().tolist() == [9, 6, 4]
    after = on.result(want_path=True)
    assert after[0] == mid[0]
    np.testing.assert_array_equal(after[1]["end_cost"], mid[1]["end_cost"])
    for p, q in zip(after[1]["paths"], mid[1]["paths"]):
        np.testing.assert_array_equal(p, q)
    s.push(b, [2, 1], first=[0, 1], count=[4, 3])                         # stream 2: 4 + 4, stream 1: 6 + 3
    assert s.frames().tolist() == [9, 9, 8]
    on.close()
    b.close()
