# -*- coding: utf-8 -*-
"""Forward scores of the isolated-word recogniser on the device (gh_forward_chain.hip: gh_chain_forward,
gh_wordstream_create_soft / _result_soft), the vocabulary posteriors and the rejection threshold on top of them.

Both sides work on the device's own likelihood matrix (fetched once per case), as tests/test_gpu_word_posteriors.py does:
  1. soft costs == the restatement (tests/word_forward_ref.py), rtol 1e-10 and +inf where it is +inf -- the tolerance the
     project holds for log P of the same arithmetic in fb_loop_kernel -- over every instantiation (N = 1 .. 8, with and
     without skip arcs, fp64 and fp32 likelihoods) at C = 3 and 21, over the chain counts {1, 3, 10, 16, 21, 64, 65, 130} at
     N = 5, and with frames scaled by 1e3; seven ragged utterances with T from {1, 2, N-1, N, 15, 16, 17, 33, 40};
  2. T == N without skip arcs has one path: the soft cost is bitwise the Viterbi cost; soft <= cost everywhere;
  3. an utterance gives bitwise the same row alone, first in a batch and last in a batch;
  4. online: `result_soft` after every push is bitwise `gh_chain_forward` of the prefix (k >= 1), for every chunking, with
     streams that sit ticks out, a reused id, a partly filled wave and several waves per stream; `result` of a soft session
     is bitwise that of a plain one;
  5. end to end: recognize(want_posteriors=True), min_confidence, online(soft=True) through push_audio;
  6. every refusal through the real library."""
import numpy as np
import pytest

import stream_endpoints_ref as S
import word_forward_ref as F

pytestmark = pytest.mark.gpu

D = 6
T_POOL = (1, 2, 15, 16, 17, 33, 40)


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


def random_model(R, rng, W, n, skip, M=2, dim=D):
    means = rng.normal(size=(W, n, M, dim)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, dim))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    return [make_hmm(R, means[i], vars_[i], w[i], F.word_trans(rng, n, skip)) for i in range(W)]


def ragged_lengths(rng, n):
    """Seven lengths from {1, 2, N-1, N, 15, 16, 17, 33, 40}: 40, 33, 17 (a wave of C = 21 then takes the unguarded run,
    T = 17 being its shortest member: 16 ordinary columns), 16 (one short of it) and three more."""
    pool = sorted({T for T in T_POOL + (n - 1, n) if T >= 1})
    return [16, 1, 40] + [int(T) for T in rng.choice(pool, size=2)] + [17, 33]


def recognizer(R, ctx, rng, W, n, skip, dtype=np.float64):
    from sr.recognition.batch import IsolatedWordRecognizer
    hmms = random_model(R, rng, W, n, skip)
    rec = IsolatedWordRecognizer(hmms, dtype=dtype, ctx=ctx)
    assert rec.gmm.M == 2 and not rec.single
    return rec, [h.transitions for h in hmms]


def check_against_restatement(hip, ctx, rec, trans, xs, dtype):
    """soft_costs of the batch against the restatement on the matrix the device computed; returns (soft, batch lengths)."""
    b = hip.Batch(ctx, xs, dtype=dtype)
    try:
        nll = np.asarray(b.loglik(rec.gmm), dtype=np.float64)            # [N, S]: the device's own numbers
        off = np.concatenate([[0], np.cumsum(b.lengths)]).astype(np.int64)
        soft = rec.soft_costs(b)                                         # (the matrix is resident: no second gh_loglik)
        want = F.soft_costs_batch(nll, off, trans)
    finally:
        b.close()
    assert soft.shape == want.shape == (len(xs), rec.W)
    np.testing.assert_array_equal(np.isposinf(soft), np.isposinf(want))
    fin = np.isfinite(want)
    assert not np.isnan(soft).any() and np.all(np.isfinite(soft[fin]))
    err = np.max(np.abs(soft[fin] - want[fin]) / np.abs(want[fin])) if fin.any() else 0.0
    print("largest relative error of the soft costs: %.3e over %d cells (%d +inf)" % (err, int(fin.sum()), int((~fin).sum())))
    np.testing.assert_allclose(soft[fin], want[fin], rtol=1e-10, atol=0)
    return soft, want


# ------------------------------------------------------------------------------------------- 1: against the restatement
SIZES = [(n, False) for n in range(1, 9)] + [(n, True) for n in range(3, 9)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,skip", SIZES)
def test_soft_costs_every_instantiation(R, hip, ctx, n, skip, dtype):
    for C in (3, 21):
        rng = np.random.default_rng(1000 * C + 10 * n + skip)
        rec, trans = recognizer(R, ctx, rng, C, n, skip, dtype)
        xs = [rng.normal(size=(T, D)) * 2.0 for T in ragged_lengths(rng, n)]
        soft, want = check_against_restatement(hip, ctx, rec, trans, xs, dtype)
        assert np.isfinite(want).any()
        if n > 1:
            assert np.all(np.isposinf(soft[1]))                          # one frame, the end row is not the start row


@pytest.mark.parametrize("C", [1, 3, 10, 16, 21, 64, 65, 130])
def test_soft_costs_every_chain_count(R, hip, ctx, C):
    n = 5
    rng = np.random.default_rng(77 + C)
    rec, trans = recognizer(R, ctx, rng, C, n, C in (16, 65))
    xs = [rng.normal(size=(T, D)) * 2.0 for T in ragged_lengths(rng, n)]
    check_against_restatement(hip, ctx, rec, trans, xs, np.float64)


def test_soft_costs_of_large_costs(R, hip, ctx):
    """Frames scaled by 1e3.  Under the reference's linear-domain underflow rule (a context's default) a cost above 745 is
    +inf; set_compat(underflow=False) keeps the likelihoods in the log domain, where these costs are finite."""
    rng = np.random.default_rng(5)
    rec, trans = recognizer(R, ctx, rng, 10, 5, True)
    xs = [rng.normal(size=(T, D)) * 2.0e3 for T in ragged_lengths(rng, 5)]
    ctx.set_compat(underflow=False)
    try:
        soft, want = check_against_restatement(hip, ctx, rec, trans, xs, np.float64)
    finally:
        ctx.set_compat(underflow=True)
    fin = np.isfinite(want)
    assert fin.sum() >= 40 and want[fin].min() > 1e5                     # log-alphas of order 1e6 and more


# ------------------------------------------------------------------------------------------- 2: against Viterbi
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_one_path_is_bitwise_the_viterbi_cost(R, hip, ctx, n):
    rng = np.random.default_rng(n)
    rec, _ = recognizer(R, ctx, rng, 10, n, False)
    xs = [rng.normal(size=(n, D)) * 2.0 for _ in range(9)]               # T == N, no skip arcs: one path per word
    b = hip.Batch(ctx, xs)
    costs = rec.costs(b)
    soft = rec.soft_costs(b)
    b.close()
    assert np.all(np.isfinite(costs))
    np.testing.assert_array_equal(soft, costs)


@pytest.mark.parametrize("n,skip", [(1, False), (3, True), (5, False), (8, True)])
def test_soft_cost_never_exceeds_the_viterbi_cost(R, hip, ctx, n, skip):
    """Against `costs(batch)` from two frames on, and against the carried session's costs for every length: the one-shot
    decode of a ONE-frame utterance is the reference's column wrap, the session (like the forward sweep) shows column 0."""
    rng = np.random.default_rng(30 + n)
    rec, _ = recognizer(R, ctx, rng, 21, n, skip)
    lens = ragged_lengths(rng, n)
    xs = [rng.normal(size=(T, D)) * 2.0 for T in lens]
    b = hip.Batch(ctx, xs)
    costs = rec.costs(b)
    soft = rec.soft_costs(b)
    on = rec.online(len(xs))
    on.push_batch(np.arange(len(xs)), b)
    _, info = on.result()
    on.close()
    b.close()
    two = np.array(lens) >= 2
    np.testing.assert_array_equal(info["costs"][two], costs[two])
    assert np.all(soft <= info["costs"]) and np.all(soft[two] <= costs[two])
    np.testing.assert_array_equal(np.isposinf(soft), np.isposinf(info["costs"]))


# ------------------------------------------------------------------------------------------- 3: batch position
def test_a_row_does_not_depend_on_the_batch(R, hip, ctx):
    rng = np.random.default_rng(12)
    rec, _ = recognizer(R, ctx, rng, 21, 5, True)
    x = rng.normal(size=(40, D)) * 2.0
    others = [rng.normal(size=(T, D)) * 2.0 for T in (3, 17, 33, 16, 9)]
    rows = []
    for xs, at in (([x], 0), ([x] + others, 0), (others + [x], len(others))):
        b = hip.Batch(ctx, xs)
        nll = b.loglik(rec.gmm)
        o = int(np.sum(b.lengths[:at]))
        rows.append((rec.soft_costs(b)[at], nll[o:o + 40].copy()))
        b.close()
    for soft, nll in rows[1:]:
        np.testing.assert_array_equal(nll, rows[0][1])                   # the same likelihoods ...
        np.testing.assert_array_equal(soft, rows[0][0])                  # ... the same row, bitwise
    assert np.all(np.isfinite(rows[0][0]))


# ------------------------------------------------------------------------------------------- 4: online
def prefix_soft(hip, ctx, rec, xs, ks, dtype=np.float64):
    """gh_chain_forward of the first ks[u] frames of every utterance, from the SAME likelihoods as a batch of the whole
    utterances: the batch is cut into [prefix | rest] pieces, so every frame keeps its row of the matrix."""
    pieces, where = [], []
    for x, k in zip(xs, ks):
        where.append(len(pieces) if k > 0 else -1)
        pieces += [p for p in (x[:k], x[k:]) if len(p)]
    b = hip.Batch(ctx, pieces, dtype=dtype)
    b.loglik(rec.gmm, fetch=False)
    soft = rec.lat.chain_forward(b)
    b.close()
    return np.array([soft[i] if i >= 0 else np.full(rec.W, np.inf) for i in where])


def run_online(hip, ctx, rec, xs, ids, n_streams, schedule, dtype=np.float64, check_plain=True):
    """Feeds utterance u to stream ids[u] in the chunks of `schedule` (a list of count vectors) from ONE resident matrix;
    after every push the soft costs of all named streams are bitwise gh_chain_forward of their prefixes."""
    b = hip.Batch(ctx, xs, dtype=dtype)
    b.loglik(rec.gmm, fetch=False)
    on = hip.WordStreamSession(ctx, rec.lat, n_streams, soft=True)
    plain = hip.WordStreamSession(ctx, rec.lat, n_streams) if check_plain else None
    pos = np.zeros(len(xs), dtype=np.int64)
    T = np.asarray(b.lengths, dtype=np.int64)
    for cnt in schedule:
        cnt = np.minimum(np.asarray(cnt, dtype=np.int64), T - pos)
        on.push(b, ids, first=pos, count=cnt)
        if plain is not None:
            plain.push(b, ids, first=pos, count=cnt)
        pos += cnt
        np.testing.assert_array_equal(on.result_soft(ids), prefix_soft(hip, ctx, rec, xs, pos, dtype))
    assert np.all(pos == T), "the schedule must feed every utterance to its end"
    if plain is not None:                                                # the cost column is not disturbed
        a, c = on.result(ids), plain.result(ids)
        np.testing.assert_array_equal(a["costs"], c["costs"])
        np.testing.assert_array_equal(a["best"], c["best"])
        with pytest.raises(hip.BackendError, match="not made by gh_wordstream_create_soft"):
            plain.result_soft(ids)
        plain.close()
    out = on.result_soft(ids)
    rest = np.setdiff1d(np.arange(n_streams), ids)
    assert np.all(np.isposinf(on.result_soft(rest)))                     # streams without frames
    on.close()
    b.close()
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("chunk", range(1, 10))
def test_carried_forward_is_bitwise_the_one_shot_forward(R, hip, ctx, chunk, dtype):
    """Chunks of 1 .. 9 frames (1: one frame at a time); three streams of 10 words x 5 states, one of them shorter than a
    word."""
    rng = np.random.default_rng(chunk)
    rec, _ = recognizer(R, ctx, rng, 10, 5, chunk % 2 == 0, dtype)
    xs = [rng.normal(size=(T, D)) * 2.0 for T in (19, 3, 12)]
    schedule = [[chunk] * 3] * (-(-19 // chunk))
    out = run_online(hip, ctx, rec, xs, np.array([4, 0, 2]), 5, schedule, dtype)
    assert np.all(np.isfinite(out[0]))
    if chunk % 2:
        assert np.all(np.isposinf(out[1]))                               # three frames, five states, no skip arcs


def test_streams_that_sit_ticks_out(R, hip, ctx):
    rng = np.random.default_rng(40)
    rec, _ = recognizer(R, ctx, rng, 10, 5, False)
    xs = [rng.normal(size=(T, D)) * 2.0 for T in (21, 20, 18, 17)]
    schedule = [[3, 0, 20, 1], [0, 0, 0, 5], [7, 9, 0, 0], [0, 1, 0, 16], [30, 30, 30, 30]]
    run_online(hip, ctx, rec, xs, np.array([1, 3, 0, 2]), 4, schedule)


@pytest.mark.parametrize("C,n_utts", [(21, 5), (65, 3)], ids=["five-streams-C21", "C65"])
def test_partly_filled_wave_and_several_waves_per_stream(R, hip, ctx, C, n_utts):
    rng = np.random.default_rng(C)
    rec, _ = recognizer(R, ctx, rng, C, 4, True)
    xs = [rng.normal(size=(T, D)) * 2.0 for T in (40, 17, 33, 16, 2)[:n_utts]]
    schedule = [[1] * n_utts, [16] * n_utts, [17] * n_utts, [40] * n_utts]
    run_online(hip, ctx, rec, xs, np.arange(n_utts)[::-1].copy(), n_utts + 2, schedule)


def test_a_reused_id_is_a_fresh_stream(R, hip, ctx):
    rng = np.random.default_rng(41)
    rec, _ = recognizer(R, ctx, rng, 10, 5, True)
    xs = [rng.normal(size=(T, D)) * 2.0 for T in (18, 25)]
    b = hip.Batch(ctx, xs)
    b.loglik(rec.gmm, fetch=False)
    used = hip.WordStreamSession(ctx, rec.lat, 2, soft=True)
    used.push(b, [1, 0], count=[11, 25])                                 # stream 1 holds part of utterance 0 ...
    used.reset([1])
    assert used.frames().tolist() == [25, 0] and np.all(np.isposinf(used.result_soft([1])))
    used.push(b, [0, 1], first=[0, 0], count=[0, 9])                     # ... and then takes utterance 1 from its start
    used.push(b, [0, 1], first=[0, 9], count=[0, 16])
    fresh = hip.WordStreamSession(ctx, rec.lat, 2, soft=True)
    fresh.push(b, [0, 1], first=[0, 0], count=[0, 9])
    fresh.push(b, [0, 1], first=[0, 9], count=[0, 16])
    np.testing.assert_array_equal(used.result_soft([1]), fresh.result_soft([1]))
    np.testing.assert_array_equal(used.result_soft([1])[0], rec.lat.chain_forward(b)[1])
    a, c = used.result([1]), fresh.result([1])
    np.testing.assert_array_equal(a["costs"], c["costs"])
    used.reset()
    assert np.all(np.isposinf(used.result_soft())) and not used.frames().any()
    used.close()
    fresh.close()
    b.close()


# ------------------------------------------------------------------------------------------- 5: end to end
A_TICK = 3200


@pytest.fixture(scope="module")
def audio(R, hip, ctx):
    """Eight 16 kHz recordings, a 3-word model on the 39 features of the front-end and the `feature_stats` normalisation of
    the recordings (as tests/test_gpu_online_words.py builds them)."""
    from sr.feature import feature_stats
    from sr.recognition.batch import IsolatedWordRecognizer
    rng = np.random.default_rng(19)
    rate = 16000
    lens = [12000, 13333, 15000, 16111, 18000, 14000, 17000, 9000]
    sigs = [S.burst_signal(rng, n, 40, [(2000, n - 2000)], freq=300.0 + 150 * i, rate=rate) for i, n in enumerate(lens)]
    norm = feature_stats(sigs, rate)
    W, n, M, dim = 3, 4, 2, 39
    trans = np.full((n, n), np.inf)
    for i in range(n):
        trans[i, i] = -np.log(0.8) if i < n - 1 else 0.0
        if i < n - 1:
            trans[i + 1, i] = -np.log(0.2)
    hmms = [make_hmm(R, rng.normal(size=(n, M, dim)), rng.uniform(0.5, 1.5, size=(n, M, dim)), rng.dirichlet(np.ones(M), size=n), trans)
            for _ in range(W)]
    return dict(sigs=sigs, norm=norm, rec=IsolatedWordRecognizer(hmms, ctx=ctx), rate=rate)


def test_recognize_with_posteriors_end_to_end(hip, ctx, audio):
    from sr.feature import features_from_signals
    from sr.recognition.batch import vocabulary_posteriors
    rec = audio["rec"]
    b = features_from_signals(audio["sigs"], audio["rate"], normalize=audio["norm"])
    xs = [np.asarray(x, dtype=np.float64) for x in b.features()]
    b.close()
    plain = rec.recognize(xs)
    assert len(plain) == 2
    words, costs, info = rec.recognize(xs, want_posteriors=True, scale=0.02)
    np.testing.assert_array_equal(words, plain[0])
    np.testing.assert_array_equal(costs, plain[1])
    assert set(info) == {"soft_costs", "posteriors", "confidence", "soft_words"}
    assert np.all(np.isfinite(info["soft_costs"])) and np.all(info["soft_costs"] <= costs)
    np.testing.assert_array_equal(info["posteriors"], vocabulary_posteriors(info["soft_costs"], 0.02))
    np.testing.assert_allclose(info["posteriors"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(info["confidence"], info["posteriors"][np.arange(len(xs)), words])
    np.testing.assert_array_equal(info["soft_words"], np.argmax(info["posteriors"], axis=1))
    assert np.all(info["confidence"] > 0.0) and np.all(info["confidence"] <= 1.0)
    above = float(info["confidence"].max()) + 1e-6
    w2, c2, _ = rec.recognize(xs, want_posteriors=True, scale=0.02, min_confidence=above)
    assert w2.tolist() == [-1] * len(xs)
    np.testing.assert_array_equal(c2, costs)
    w3, _, _ = rec.recognize(xs, want_posteriors=True, scale=0.02, min_confidence=float(info["confidence"].min()))
    np.testing.assert_array_equal(w3, words)                             # (at the threshold a word is kept)
    with pytest.raises(ValueError):
        rec.recognize(xs, min_confidence=0.5)


def test_online_soft_through_push_audio_equals_the_offline_call(hip, ctx, audio):
    """The streaming front-end's frames are bitwise the one-shot front-end's; their likelihoods are computed per tick, i.e.
    in other batches, which the project's tests hold to 1e-12 relative in a cost.  A soft cost is a sum of the same
    numbers: 1e-10, the tolerance of log P.  A posterior moves by at most the change of its z differences,
    2 scale max|soft| 1e-10."""
    from sr.feature import StreamingFrontend, features_from_signals
    rec, sigs, rate = audio["rec"], audio["sigs"], audio["rate"]
    scale = 0.02
    b = features_from_signals(sigs, rate, normalize=audio["norm"])
    ref_costs = rec.costs(b)
    ref_post, ref_soft = rec.posteriors(b, scale=scale)
    b.close()
    fe = StreamingFrontend(8, rate, normalize=audio["norm"], max_chunk=A_TICK)
    on = rec.online(8, frontend=fe, soft=True, scale=scale)
    pos = [0] * 8
    lengths = [A_TICK, 777, 1600, 0, 2999, 161]
    t = 0
    while any(p < len(s) for p, s in zip(pos, sigs)):
        live = [k for k in range(8) if pos[k] < len(sigs[k])]
        chunks = []
        for k in live:
            c = lengths[(k + t) % len(lengths)]
            chunks.append(sigs[k][pos[k]:pos[k] + c])
            pos[k] += len(chunks[-1])
        on.push_audio(live, chunks, [pos[k] >= len(sigs[k]) for k in live])
        t += 1
    words, info = on.result(np.arange(8))
    np.testing.assert_array_equal(words, np.argmin(ref_costs, axis=1))
    np.testing.assert_allclose(info["soft_costs"], ref_soft, rtol=1e-10)
    np.testing.assert_allclose(info["posteriors"], ref_post, rtol=0, atol=2 * scale * np.abs(ref_soft).max() * 1e-10)
    np.testing.assert_array_equal(info["soft_words"], np.argmax(ref_post, axis=1))
    np.testing.assert_array_equal(info["confidence"], info["posteriors"][np.arange(8), words])
    fw, fi = on.finish(np.arange(8))
    np.testing.assert_array_equal(fi["posteriors"], info["posteriors"])
    w0, i0 = on.result([0])
    assert w0[0] == -1 and np.all(np.isposinf(i0["soft_costs"])) and i0["confidence"][0] == 0.0 and i0["soft_words"][0] == -1
    on.close()
    fe.close()
    plain = rec.online(2)
    assert set(plain.result()[1]) == {"costs", "frames"}                # without soft=True everything is as before
    plain.close()


# ------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_through_the_real_library(R, hip, ctx):
    from sr.recognition.batch import IsolatedWordRecognizer
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    rng = np.random.default_rng(3)
    W, n = 4, 3
    hmms = random_model(R, rng, W, n, False)
    wt = [h.transitions for h in hmms]
    rec = IsolatedWordRecognizer(hmms, ctx=ctx)
    b = hip.Batch(ctx, [rng.normal(size=(5, D)), rng.normal(size=(4, D))])
    with pytest.raises(hip.BackendError, match="gh_loglik has not been run"):
        rec.lat.chain_forward(b)                                         # a batch without likelihoods
    b.loglik(rec.gmm, fetch=False)
    ok = rec.lat.chain_forward(b)
    assert ok.shape == (2, W) and np.all(np.isfinite(ok))
    empty = hip.Batch(ctx, [])
    assert rec.lat.chain_forward(empty).shape == (0, W)                  # U = 0
    empty.close()

    def stacked(trans_list):
        sizes = [len(t) for t in trans_list]
        o = np.concatenate([[0], np.cumsum(sizes)])
        to, frm, cost = [], [], []
        for i, t in enumerate(trans_list):
            a, c = np.nonzero(~np.isinf(t))
            to.append(a + o[i]); frm.append(c + o[i]); cost.append(t[a, c])
        return dict(row_state=np.arange(o[-1], dtype=np.int32), arc_to=np.concatenate(to), arc_from=np.concatenate(frm),
                    arc_cost=np.concatenate(cost), start_rows=o[:-1], end_rows=o[1:] - 1)

    cases = [([packed_loop_lattice(wt, n, 0.0)[0]], "word-loop grammar"),
             ([packed_bigram_lattice(wt, n, rng.uniform(0.5, 3.0, size=(W, W)), None)[0]], "bigram grammar"),
             ([packed_lattice(wt, n, [list(range(W))] * 3)[0]], "K-layer word lattice"),
             ([stacked([F.word_trans(rng, 3), F.word_trans(rng, 4), F.word_trans(rng, 3)])], "chains of unequal length"),
             ([stacked([F.word_trans(rng, 12)] * 2)], "chains of 12 states"),
             ([stacked(wt), stacked(wt)], "several graphs")]
    for graphs, sentence in cases:
        lat = hip.Lattices(ctx, graphs)
        with pytest.raises(hip.Unsupported, match=sentence):
            lat.chain_forward(b)
        with pytest.raises(hip.Unsupported, match=sentence):
            hip.WordStreamSession(ctx, lat, 4, soft=True)
        lat.close()
    lat = hip.Lattices.from_transcripts(ctx, wt, n, label_seqs=[[0], [1, 2]])
    with pytest.raises(hip.Unsupported, match="made from transcripts"):
        lat.chain_forward(b)
    lat.close()
    lat = hip.Lattices(ctx, [stacked(wt)])
    np.testing.assert_array_equal(lat.chain_forward(b), ok)              # (the same graph without a beam is taken)
    lat.set_beam(3)
    with pytest.raises(hip.Unsupported, match="rank beam"):
        lat.chain_forward(b)
    with pytest.raises(hip.Unsupported, match="rank beam"):
        hip.WordStreamSession(ctx, lat, 4, soft=True)
    lat.close()
    wide = hip.Lattices(ctx, [stacked(wt + [F.word_trans(rng, n)])])     # one word more than the model has states for
    with pytest.raises(hip.BackendError, match="uses state"):
        wide.chain_forward(b)
    wide.close()
    plain = hip.WordStreamSession(ctx, rec.lat, 2)
    with pytest.raises(hip.BackendError, match="not made by gh_wordstream_create_soft"):
        plain.result_soft()
    plain.close()
    soft = hip.WordStreamSession(ctx, rec.lat, 2, soft=True)
    with pytest.raises(hip.BackendError):
        soft.result_soft([2])                                            # an id out of range
    soft.close()
    b.close()
    single = []
    for h in hmms:
        m = R.HMM(n)
        m.mu, m.sigma, m.transitions = h.mu.copy(), h.sigma.copy(), h.transitions.copy()
        m.use_gmm, m.gmm_states = False, None
        single.append(m)
    srec = IsolatedWordRecognizer(single, ctx=ctx)
    xs = [rng.normal(size=(6, D))]
    with pytest.raises(hip.Unsupported, match="one Gaussian per state"):
        srec.recognize(xs, want_posteriors=True)
    with pytest.raises(hip.Unsupported):
        srec.online(2, soft=True)
    assert len(srec.recognize(xs)) == 2
