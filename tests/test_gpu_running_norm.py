# -*- coding: utf-8 -*-
"""The causal running mean / variance normalisation on the GPU (csrc/gh_norm_running.hip).

(a) `Batch.running_norm` against the numpy restatement (tests/running_norm_ref.py), BITWISE: every operation of the rule
    is one correctly rounded fp64 operation, evaluated in the order written without contraction, so numpy scalars round
    the same.  This rests on the device's fp64 division and square root being correctly rounded.
(b) - (e) hold the stream to the offline pass, bitwise: the same kernel runs on both sides and the sums are strictly
    sequential in frame order, so this does not depend on (a)'s assumption about the square root.
(b) a stream's concatenated output = `features_from_signals([signal], normalize=norm)` of its utterance alone, however
    the audio was cut: 5 streams interleaved, one-sample chunks around a frame boundary, pushes that emit no frame, the
    final flush on a chunk of its own.
(c) a reused stream id: per="utterance" starts every utterance from the prior; per="stream" carries (S, Q, c) from one
    utterance into the next until `reset_stats`; `norm_frames` after every push.
(d) a refused push (an id twice, a chunk over max_chunk) moves neither `samples` nor `norm_frames`, in the package and in
    the library, and the next push emits what it would have.
(e) audio in, words out: `push_audio` through a front-end with a RunningNorm decodes exactly like `decode_batch` of
    `features_from_signals(..., normalize=norm)`.  The one-shot MFCC kernel pairs frames inside their utterance, as the
    stream does, so EVERY utterance of the batch of all signals is held to exact equality -- the one behind an odd number
    of frames too -- and to the decode of its own one-utterance batch."""
import numpy as np
import pytest

from conftest import load_golden
from running_norm_ref import running_norm

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


# ------------------------------------------------------------------ (a) the offline kernel against the restatement
LENS = [1, 2, 3, 64, 65, 257]


@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(2300)
    D = 39
    utts = [rng.normal(size=(T, D)) * rng.uniform(0.5, 8.0, size=D) + rng.normal(size=D) * 4.0 for T in LENS]
    for x in utts:
        x[:, 11] = -3.5                                    # a constant coefficient: the floor
        x[:, 20] = rng.normal(size=len(x)) * 1e6 + 3e6     # values of 1e6 magnitude
    mean, std = rng.normal(size=D) * 2.0, rng.uniform(0.5, 4.0, size=D)
    return utts, mean, std


@pytest.mark.parametrize("dtype", DTYPES)
def test_offline_pass_equals_the_restatement_bitwise(hip, ctx, synthetic, dtype):
    utts, mean, std = synthetic
    for P in (0, 1, 100):
        b = hip.Batch(ctx, utts, dtype=dtype)
        assert b.running_norm(mean, std, prior_frames=P, min_std=0.1) is b
        got = b.features()
        for u, x in enumerate(utts):
            want, _ = running_norm(x, mean, std, P, 0.1, dtype=dtype)
            assert got[u].dtype == dtype and np.all(np.isfinite(got[u]))
            np.testing.assert_array_equal(got[u], want, err_msg="P = %d, utterance of %d frames" % (P, len(x)))
            if P == 0:                                     # no prior: the first frame is its own mean
                np.testing.assert_array_equal(got[u][0], 0.0)
        b.close()


def test_offline_pass_takes_any_dimension_and_forgets_likelihoods(hip, ctx):
    rng = np.random.default_rng(2301)
    utts = [rng.normal(size=(T, 5)) * 3.0 + 1.0 for T in (7, 1, 130)]
    mean, std = rng.normal(size=5), rng.uniform(0.5, 2.0, size=5)
    for dtype in DTYPES:
        b = hip.Batch(ctx, utts, dtype=dtype)
        b.running_norm(mean, std, prior_frames=3, min_std=0.5)
        for x, f in zip(utts, b.features()):
            np.testing.assert_array_equal(f, running_norm(x, mean, std, 3, 0.5, dtype=dtype)[0])
        with pytest.raises(ValueError):
            b.running_norm(mean[:4], std[:4])
        for bad in (dict(prior_frames=-1), dict(prior_frames=1.5), dict(min_std=0.0), dict(min_std=1.25), dict(min_std=float("nan"))):
            with pytest.raises(hip.BackendError):          # the library refuses on its own
                b.running_norm(mean, std, **bad)
        with pytest.raises(hip.BackendError):
            b.running_norm(mean, np.where(np.arange(5) == 2, 0.0, std))
        b.close()
    # likelihoods the batch holds belong to the features it had
    S, M = 3, 2
    gmm = hip.PackedGMM(ctx, rng.normal(size=(S, M, 5)), rng.uniform(0.5, 1.5, size=(S, M, 5)), rng.dirichlet(np.ones(M), size=S))
    b = hip.Batch(ctx, utts)
    b.loglik(gmm)
    b.running_norm(mean, std, prior_frames=3)
    assert b.S is None
    fresh = hip.Batch(ctx, [f.copy() for f in b.features()])
    np.testing.assert_array_equal(b.loglik(gmm), fresh.loglik(gmm))
    b.close(), fresh.close(), gmm.close()


# ------------------------------------------------------------------ the recorded audio and its offline references
WHICH = [3, 4, 8, 5, 6]                 # 161 samples (2 frames), 400 (3), 800 (5, silence: the floor), 4 001 (26), 16 000 (100)


@pytest.fixture(scope="module")
def g15():
    g = load_golden("G15_mfcc")
    return {i: g["signal%d" % i] for i in WHICH}


@pytest.fixture(scope="module")
def prior(g15):
    from sr.feature import feature_stats
    return feature_stats([g15[5], g15[6]], 16000)


def make_norm(prior, per="utterance"):
    from sr.feature import RunningNorm
    return RunningNorm(prior, prior_frames=20, min_std=0.1, per=per)


@pytest.fixture(scope="module")
def offline(hip, ctx, g15, prior):
    """Computed once: signal -> dtype -> (`features_from_signals([signal], normalize=norm)`, the raw mode-1 features)."""
    from sr.feature import features_from_signals
    out = {}
    for i in WHICH:
        out[i] = {}
        for dt in DTYPES:
            b = features_from_signals([g15[i]], 16000, dtype=dt, normalize=make_norm(prior))
            r = hip.Batch(ctx, pcm=[g15[i]], sample_rate=16000, frontend_mode=1, dtype=dt)
            out[i][dt] = (b.features()[0].copy(), r.features()[0].copy())
            b.close(), r.close()
    return out


def test_offline_features_are_the_rule_on_the_raw_features(offline, prior):
    for i in WHICH:
        for dt in DTYPES:
            got, raw = offline[i][dt]
            assert got.dtype == dt and got.shape == raw.shape
            np.testing.assert_array_equal(got, running_norm(raw, prior[0], prior[1], 20, 0.1, dtype=dt)[0])


def feed(fe, rng, signals, plans, ids_of):
    """signals[k] goes to stream ids_of[k] in chunks of plans[k] samples, the last chunk with the end flag; all streams
    share the pushes, in an order drawn per push.  Checks `norm_frames` after every push; returns each concatenated output."""
    K = len(signals)
    pos, step, got, emitted = [0] * K, [0] * K, [[] for _ in range(K)], fe.norm_frames
    while any(step[k] < len(plans[k]) for k in range(K)):
        live = [int(k) for k in rng.permutation(K) if step[k] < len(plans[k])]
        chunks = [signals[k][pos[k]:pos[k] + plans[k][step[k]]] for k in live]
        end = [step[k] == len(plans[k]) - 1 for k in live]
        b = fe.push([ids_of[k] for k in live], chunks, end)
        for k, f, n in zip(live, b.features(), b.lengths):
            got[k].append(f.copy())
            emitted[ids_of[k]] += n
            pos[k] += plans[k][step[k]]
            step[k] += 1
        b.close()
        assert fe.norm_frames.tolist() == emitted.tolist()
        np.testing.assert_array_equal(fe.backend.norm_frames(), emitted)
    assert pos == [len(s) for s in signals]
    return [np.concatenate(g) for g in got]


def random_cut(rng, n):
    out = []
    while sum(out) < n:
        out.append(0 if rng.random() < 0.2 else int(min(rng.integers(0, 701), n - sum(out))))
    return out


# ------------------------------------------------------------------ (b) streaming against offline
@pytest.mark.parametrize("dtype", DTYPES)
def test_streams_equal_the_offline_pass_bitwise(g15, prior, offline, dtype):
    from sr.feature import StreamingFrontend
    rng = np.random.default_rng(2302)
    signals = [g15[i] for i in WHICH]
    # frame t is complete at t * 160 + 400 samples: one-sample chunks across 720 (frame 2) and 880 (frame 3, which
    # completes a pair and makes the first frames final); the end flag on an empty chunk of its own for three streams
    plans = [[161],
             [160, 0, 240, 0],
             [37] * 21 + [23, 0],
             [718, 1, 1, 1, 1, 156, 1, 1, 1, 1] + random_cut(rng, 4001 - 882),
             random_cut(rng, 16000) + [0]]
    assert [sum(p) for p in plans] == [len(s) for s in signals]
    fe = StreamingFrontend(5, 16000, normalize=make_norm(prior), max_chunk=16000, dtype=dtype)
    zero_frame_pushes = fe.frames_ready(718) == fe.frames_ready(719)
    assert zero_frame_pushes
    got = feed(fe, rng, signals, plans, [4, 2, 0, 3, 1])
    for i, f in zip(WHICH, got):
        assert f.dtype == dtype
        np.testing.assert_array_equal(f, offline[i][dtype][0], err_msg="signal %d" % i)
    fe.close()


# ------------------------------------------------------------------ (c) a reused stream id
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_reused_id_per_utterance_and_per_stream(g15, prior, offline, dtype):
    from sr.feature import StreamingFrontend
    rng = np.random.default_rng(2303)
    first, second = g15[5], g15[6]
    # per="utterance": reset clears the statistics -- the second utterance is what a fresh front-end emits
    fe = StreamingFrontend(3, 16000, normalize=make_norm(prior), max_chunk=16000, dtype=dtype)
    a = feed(fe, rng, [first], [random_cut(rng, len(first))], [1])[0]
    np.testing.assert_array_equal(a, offline[5][dtype][0])
    assert fe.norm_frames.tolist() == [0, 26, 0]
    fe.reset([1])
    assert fe.norm_frames.tolist() == [0, 0, 0] and fe.backend.norm_frames().tolist() == [0, 0, 0]
    b = feed(fe, rng, [second], [random_cut(rng, len(second))], [1])[0]
    fresh = StreamingFrontend(1, 16000, normalize=make_norm(prior), max_chunk=16000, dtype=dtype)
    c = feed(fresh, rng, [second], [[len(second)]], [0])[0]
    np.testing.assert_array_equal(b, c)
    np.testing.assert_array_equal(b, offline[6][dtype][0])
    fe.close(), fresh.close()
    # per="stream": the second utterance starts from the sums of the first
    fe = StreamingFrontend(3, 16000, normalize=make_norm(prior, per="stream"), max_chunk=16000, dtype=dtype)
    a = feed(fe, rng, [first], [random_cut(rng, len(first))], [1])[0]
    np.testing.assert_array_equal(a, offline[5][dtype][0])
    fe.reset([1])
    assert fe.samples.tolist() == [0, 0, 0] and fe.norm_frames.tolist() == [0, 26, 0]
    np.testing.assert_array_equal(fe.backend.norm_frames(), [0, 26, 0])
    b = feed(fe, rng, [second], [random_cut(rng, len(second))], [1])[0]
    assert fe.norm_frames.tolist() == [0, 126, 0]
    _, state = running_norm(offline[5][dtype][1], prior[0], prior[1], 20, 0.1, dtype=dtype)
    want, _ = running_norm(offline[6][dtype][1], prior[0], prior[1], 20, 0.1, dtype=dtype, state=state)
    np.testing.assert_array_equal(b, want)
    assert not np.array_equal(b, offline[6][dtype][0])     # (the carried sums do change the output)
    # ... until reset_stats: the id is a fresh front-end again
    fe.reset([1])
    fe.reset_stats([1])
    assert fe.norm_frames.tolist() == [0, 0, 0] and fe.backend.norm_frames().tolist() == [0, 0, 0]
    c = feed(fe, rng, [second], [random_cut(rng, len(second))], [1])[0]
    np.testing.assert_array_equal(c, offline[6][dtype][0])
    fe.close()


# ------------------------------------------------------------------ (d) a refused push
def test_a_refused_push_moves_nothing(hip, g15, prior, offline):
    from sr.feature import StreamingFrontend
    sig = g15[5]
    fe = StreamingFrontend(2, 16000, normalize=make_norm(prior, per="stream"), max_chunk=2500)
    parts = [fe.push([1], [sig[:2000]])]
    samples, frames = fe.samples, fe.norm_frames
    assert samples.tolist() == [0, 2000] and frames.tolist() == [0, 8]
    x = sig[2000:4001]
    for ids, chunks in (([1, 1], [x, x]),                                   # an id named twice
                        ([0, 1], [sig[:2501], x])):                         # a chunk above max_chunk
        with pytest.raises(ValueError):
            fe.push(ids, chunks)
    # ... and the library on its own (the raw binding)
    with pytest.raises(hip.BackendError):
        fe.backend.push([1, 1], np.concatenate([x, x]), [0, len(x), 2 * len(x)])
    with pytest.raises(hip.BackendError):
        fe.backend.push([0, 1], np.concatenate([sig[:2501], x]), [0, 2501, 2501 + len(x)])
    assert fe.samples.tolist() == samples.tolist() and fe.norm_frames.tolist() == frames.tolist()
    np.testing.assert_array_equal(fe.backend.samples(), samples)
    np.testing.assert_array_equal(fe.backend.norm_frames(), frames)
    parts.append(fe.push([1], [x], [True]))                                 # the next push emits what it would have
    np.testing.assert_array_equal(np.concatenate([p.features()[0] for p in parts]), offline[5][np.float64][0])
    assert fe.norm_frames.tolist() == [0, 26]
    for p in parts:
        p.close()
    fe.close()


def test_the_library_refuses_a_bad_rule_before_it_allocates(hip, ctx, prior):
    mean, std = prior
    for kw in (dict(prior_frames=-1), dict(prior_frames=0.5), dict(prior_frames=float("inf")), dict(min_std=0.0), dict(min_std=2.0),
               dict(prior=(mean, -std)), dict(prior=(np.where(np.arange(39) == 4, np.nan, mean), std))):
        with pytest.raises(hip.BackendError):
            hip.RunningStreamFrontend(ctx, 2, **dict(dict(prior=prior), **kw))
    fe = hip.StreamFrontend(ctx, 2)                                         # without the rule: nothing to clear, zeros
    fe.reset(None)
    assert hip.RunningStreamFrontend.norm_frames(fe).tolist() == [0, 0]
    hip.RunningStreamFrontend.reset_stats(fe, None)
    fe.close()


# ------------------------------------------------------------------ (e) end to end: audio in, words out
TICK = 3200


def burst_signal(rng, n, sigma, bursts, amp=4000.0, freq=440.0, rate=8000):
    t = np.arange(n) / rate
    x = rng.normal(0.0, sigma, size=n) if sigma > 0 else np.zeros(n)
    for a, b in bursts:
        x[a:b] += amp * np.sin(2 * np.pi * freq * t[a:b])
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def make_hmm(R, means, vars_, w, trans):
    h = R.HMM(means.shape[0])
    h.gmm_states = []
    for s in range(means.shape[0]):
        g = R.GMM(means[s][0].copy(), vars_[s][0].copy(), len(w[s]))
        g.update_models(means[s].copy(), vars_[s].copy(), w[s].copy())
        h.gmm_states.append(g)
    h.transitions = trans.copy()
    h.mu, h.sigma = means[:, 0].copy(), vars_[:, 0].copy()
    return h


def ticks_of(sigs):
    for t in range(max(-(-len(s) // TICK) for s in sigs)):
        live = [k for k, s in enumerate(sigs) if t * TICK < len(s)]
        yield live, [sigs[k][t * TICK:(t + 1) * TICK] for k in live], [(t + 1) * TICK >= len(sigs[k]) for k in live]


def test_push_audio_decodes_like_the_offline_features(hip, ctx):
    import sr.recognition as R
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(17)
    rate = 16000
    lens = [8000, 11111, 14000, 17777, 20000, 24000]                       # 0.5 .. 1.5 s
    sigs = [burst_signal(rng, n, 40, [(n // 4, n // 2), (5 * n // 8, 7 * n // 8)], freq=300.0 + 150 * i, rate=rate)
            for i, n in enumerate(lens)]
    norm = make_norm(feature_stats(sigs, rate))
    W, n, M, D = 3, 4, 2, 39
    trans = np.full((n, n), np.inf)
    for i in range(n):
        trans[i, i] = -np.log(0.8) if i < n - 1 else 0.0
        if i < n - 1:
            trans[i + 1, i] = -np.log(0.2)
    hmms = [make_hmm(R, rng.normal(size=(n, M, D)), rng.uniform(0.5, 1.5, size=(n, M, D)), rng.dirichlet(np.ones(M), size=n), trans)
            for _ in range(W)]
    dec = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
    b = features_from_signals(sigs, rate, normalize=norm)
    ref_words, ref = dec.decode_batch(b)
    frames, starts = b.lengths.tolist(), b.offsets[:-1].tolist()
    b.close()
    fe = StreamingFrontend(6, rate, normalize=norm, max_chunk=TICK)
    on = dec.online(6, max_frames=max(frames), frontend=fe)
    for ids, chunks, end in ticks_of(sigs):
        on.push_audio(ids, chunks, end)
    assert on.frames.tolist() == frames and fe.samples.tolist() == lens and fe.norm_frames.tolist() == frames
    words, info = on.result(np.arange(6))
    assert all(len(w) >= 1 for w in words)
    n_end = info["end_cost"].shape[1]
    ref_cost = np.asarray(ref["end_cost_flat"]).reshape(6, n_end)
    assert any(st % 2 for st in starts)                    # an utterance behind an odd number of frames is among them
    for u in range(6):                                     # the batch of all signals: the frame pairs are the stream's
        assert words[u] == ref_words[u]
        assert info["best_end"][u] == ref["best_end"][u]
        np.testing.assert_array_equal(info["end_cost"][u], ref_cost[u])
    for u, s in enumerate(sigs):                           # every utterance against the decode of its own batch
        b1 = features_from_signals([s], rate, normalize=norm)
        w1, r1 = dec.decode_batch(b1)
        b1.close()
        assert words[u] == w1[0]
        assert info["best_end"][u] == r1["best_end"][0]
        np.testing.assert_array_equal(info["end_cost"][u], np.asarray(r1["end_cost_flat"]).reshape(-1))
    # a new recording on the decoder: `reset` clears the statistics as well, whatever `per` says
    on.reset([2])
    assert fe.samples[2] == 0 and on.frames[2] == 0 and fe.norm_frames[2] == 0
    for ids, chunks, end in ticks_of([sigs[0]]):
        on.push_audio([2], chunks, end)
    words2, info2 = on.result([2])
    assert words2 == words[:1]
    np.testing.assert_array_equal(info2["end_cost"][0], info["end_cost"][0])
    on.close()
    fe.close()
