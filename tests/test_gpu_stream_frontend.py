# -*- coding: utf-8 -*-
"""The streaming MFCC / delta front-end on the GPU (csrc/gh_mfcc_stream.hip).

The contract is BITWISE: whatever way a stream's audio is cut into chunks, its concatenated frames are the one-shot
front-end's (`_hip.Batch(ctx, pcm=[signal], frontend_mode=1)`) for that utterance alone, in both dtypes -- same kernel
arithmetic, frames paired by their index inside the utterance by both.  Against the numpy oracle the streamed features are
held to the rtol = atol = 1e-7 that test_gpu_api.py holds `features_from_signals` to.  The fixed normalisation is one IEEE
subtraction and one division in fp64 on the dtype-rounded value, so it is compared bitwise with numpy as well."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import ref_numpy as O
from stream_frontend_ref import raw_stack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@pytest.fixture(scope="module")
def g15():
    g = load_golden("G15_mfcc")
    return {i: g["signal%d" % i] for i in range(int(g["n"]))}, {i: int(g["rate%d" % i]) for i in range(int(g["n"]))}


@pytest.fixture(scope="module")
def one_shot(hip, ctx, g15):
    """The reference of the bitwise tests, computed once: signal index -> dtype -> the mode-1 features of that utterance alone."""
    sigs, rates = g15
    out = {}
    for i in (3, 4, 5, 6, 7, 8):
        out[i] = {}
        for dt in (np.float64, np.float32):
            b = hip.Batch(ctx, pcm=[sigs[i]], sample_rate=rates[i], frontend_mode=1, dtype=dt)
            out[i][dt] = b.features()[0].copy()
            b.close()
    return out


def cut(rng, n, how):
    """Chunk lengths that sum to n."""
    if how == "whole":
        return [n]
    if isinstance(how, int):
        return [min(how, n - k) for k in range(0, n, how)]
    out = []                                               # random 0 .. 700 with zeros
    while sum(out) < n:
        out.append(0 if rng.random() < 0.2 else int(min(rng.integers(0, 701), n - sum(out))))
    return out


def stream_all(fe, rng, signals, plans, end_alone, ids_of=None):
    """Feed signals[k] to stream ids_of[k] with the chunk lengths plans[k], all streams in the same push calls, ids permuted
    per push; end_alone[k]: the end flag comes on an empty chunk of its own instead of on the last one.  Checks the frames
    of every push against `frames_ready`; returns the concatenated output per signal."""
    K = len(signals)
    ids_of = list(range(K)) if ids_of is None else ids_of
    plans = [list(p) + ([0] if alone else []) for p, alone in zip(plans, end_alone)]
    pos, step, got = [0] * K, [0] * K, [[] for _ in range(K)]
    while any(step[k] < len(plans[k]) for k in range(K)):
        live = [int(k) for k in rng.permutation(K) if step[k] < len(plans[k])]
        chunks = [signals[k][pos[k]:pos[k] + plans[k][step[k]]] for k in live]
        end = [step[k] == len(plans[k]) - 1 for k in live]
        ids = [ids_of[k] for k in live]
        before = fe.samples[ids]
        b = fe.push(ids, chunks, end)
        after = fe.samples[ids]
        assert after.tolist() == [pos[k] + plans[k][step[k]] for k in live]
        want = fe.frames_ready(after, end) - fe.frames_ready(before)
        assert b.lengths.tolist() == list(want) and b.D == 39 and b.U == len(live)
        for k, f in zip(live, b.features()):
            got[k].append(f.copy())
            pos[k] += plans[k][step[k]]
            step[k] += 1
        b.close()
    assert pos == [len(s) for s in signals]
    return [np.concatenate(g) for g in got]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_streams_equal_the_one_shot_front_end_bitwise(hip, ctx, g15, one_shot, dtype):
    from sr.feature import StreamingFrontend
    sigs, rates = g15
    rng = np.random.default_rng(15)
    which = [3, 4, 8, 5, 6, 5]          # 161 samples (2 frames), 400 (3), 800 (5: an odd tail pair), 4 001, 16 000, 4 001 again
    hows = ["whole", 160, 37, "random", "random", 37]
    alone = [False, True, False, True, False, True]
    signals = [sigs[i] for i in which]
    plans = [cut(rng, len(s), h) for s, h in zip(signals, hows)]
    assert any(0 in p for p in plans)
    fe = StreamingFrontend(6, 16000, max_chunk=16000, dtype=dtype)
    got = stream_all(fe, rng, signals, plans, alone)
    for i, f in zip(which, got):
        assert f.dtype == dtype
        np.testing.assert_array_equal(f, one_shot[i][dtype], err_msg="signal %d" % i)
    fe.close()
    # 8 kHz: frames of 200 samples, window padded to 256 (pad_left = 28), in a front-end of its own
    fe = StreamingFrontend(1, 8000, max_chunk=3000, dtype=dtype)
    for how, al in (("random", True), (37, False), ("whole", False)):
        f7 = stream_all(fe, rng, [sigs[7]], [cut(rng, 3000, how)], [al])[0]
        np.testing.assert_array_equal(f7, one_shot[7][dtype])
        fe.reset()
    fe.close()
    if dtype == np.float64:             # ... and the oracle, at the tolerance test_gpu_api.py holds features_from_signals to
        checked = 0
        for i, f in zip(which + [7], got + [f7]):
            ceps = O.mfcc_features_signal(sigs[i], rates[i])[1]
            np.testing.assert_allclose(f, raw_stack(ceps), rtol=1e-7, atol=1e-7)
            # standardised as well, where the reference's standardize is defined: no constant column (two frames have a
            # constant delta track, signal 8 is silence) -- the restriction test_gpu_api.py makes for the same pair
            if np.all(np.std(raw_stack(ceps), axis=0) > 0):
                np.testing.assert_allclose(O.standardize(f), O.stack_features(ceps), rtol=1e-7, atol=1e-7)
                checked += 1
        assert checked >= 4                                # signals 5 (twice), 6 and 7


def test_normalisation_is_the_fixed_affine_map(hip, ctx, g15, one_shot):
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    sigs, _ = g15
    rng = np.random.default_rng(16)
    train = [sigs[5], sigs[6]]
    mean, std = feature_stats(train, 16000)
    raw = np.concatenate([one_shot[5][np.float64], one_shot[6][np.float64]])
    np.testing.assert_array_equal(mean, raw.mean(axis=0))
    np.testing.assert_array_equal(std, raw.std(axis=0))
    for dtype in (np.float64, np.float32):
        fe = StreamingFrontend(3, 16000, normalize=(mean, std), max_chunk=16000, dtype=dtype)
        got = stream_all(fe, rng, [sigs[8], sigs[5], sigs[4]], [cut(rng, 800, 160), cut(rng, 4001, "random"), cut(rng, 400, 37)],
                         [False, True, False])
        fe.close()
        # offline, all in ONE batch: the MFCC kernel pairs frames inside their utterance, so an utterance is bitwise what it
        # is alone wherever it stands (here behind 5 frames, and behind 5 + 26)
        off = features_from_signals([sigs[8], sigs[5], sigs[4]], 16000, dtype=dtype, normalize=(mean, std))
        for i, f, o in zip((8, 5, 4), got, off.features()):
            # the definition: the raw value rounded to the dtype, (x - mean) / std in fp64, rounded to the dtype
            want = ((one_shot[i][dtype].astype(np.float64) - mean) / std).astype(dtype)
            np.testing.assert_array_equal(f, want)
            np.testing.assert_array_equal(o, f)            # offline == streamed, bitwise
        off.close()
    # gh_batch_affine on an fp32 batch of arbitrary features
    x = (rng.normal(size=(50, 39)) * 7).astype(np.float32)
    b = hip.Batch(ctx, [x[:20], x[20:]], dtype=np.float32)
    b.affine(mean, std)
    np.testing.assert_array_equal(np.concatenate(b.features()), ((x.astype(np.float64) - mean) / std).astype(np.float32))
    with pytest.raises(ValueError):
        b.affine(mean[:13], std[:13])
    b.close()
    # the default of features_from_signals is unchanged: per-utterance standardisation
    d = features_from_signals([sigs[5]], 16000)
    np.testing.assert_allclose(d.features()[0], O.standardize(one_shot[5][np.float64]), rtol=1e-9, atol=1e-9)
    d.close()


def test_reset_and_refusals(hip, ctx, g15, one_shot):
    from sr.feature import StreamingFrontend
    sigs, _ = g15
    fe = StreamingFrontend(3, 16000, max_chunk=4001)
    a = fe.push([1], [sigs[8][:500]])
    assert a.lengths.tolist() == [0]
    a.close()
    fe.reset([1])                                          # the id takes another utterance: nothing of the first is left
    parts = []
    for lo, hi, end in ((0, 1000, False), (1000, 4001, True)):
        b = fe.push([2, 1], [sigs[5][:0], sigs[5][lo:hi]], [False, end])
        parts.append(b.features()[1].copy())
        b.close()
    np.testing.assert_array_equal(np.concatenate(parts), one_shot[5][np.float64])
    before = fe.samples
    assert before.tolist() == [0, 4001, 0]
    x = sigs[8]
    for ids, chunks, end in (([0, 0], [x, x], None),                       # an id named twice
                             ([0, 3], [x, x], None),                       # an id out of range
                             ([0, 2], [x, sigs[6][:4002]], None),          # a chunk over max_chunk
                             ([0, 1], [x, x], None),                       # audio after the end
                             ([0], [x[:160]], [True]),                     # an end with fewer than 2 frames
                             ([2], [x[:0]], [True]),                       # ... and one without a sample
                             ([0], [x.astype(np.float32)], None)):         # a dtype that is not int16
        with pytest.raises(ValueError):
            fe.push(ids, chunks, end)
        assert fe.samples.tolist() == before.tolist()
        np.testing.assert_array_equal(fe.backend.samples(), before)        # ... nor in the library
    # the library refuses on its own as well (the raw binding), and moves nothing
    with pytest.raises(hip.BackendError):
        fe.backend.push([0, 0], np.zeros(20, dtype=np.int16), [0, 10, 20])
    with pytest.raises(hip.BackendError):
        fe.backend.push([1], np.zeros(20, dtype=np.int16), [0, 20])        # ended
    with pytest.raises(hip.BackendError):
        fe.backend.push([0], np.zeros(160, dtype=np.int16), [0, 160], [1])
    np.testing.assert_array_equal(fe.backend.samples(), before)
    b = fe.push([0], [x], [True])                                          # the refused streams are where they were
    np.testing.assert_array_equal(b.features()[0], one_shot[8][np.float64])
    b.close()
    fe.close()


# ------------------------------------------------------------------ end to end: audio in, words out
TICK = 3200


@pytest.fixture(scope="module")
def e2e(hip, ctx):
    import sr.recognition as R
    from sr.feature import feature_stats, features_from_signals
    from sr.recognition.batch import ContinuousDecoder
    from test_gpu_api import make_hmm
    from test_gpu_audio_capture import burst_signal
    rng = np.random.default_rng(17)
    rate = 16000
    lens = [8000, 11111, 14000, 17777, 20000, 24000]                       # 0.5 .. 1.5 s
    sigs = [burst_signal(rng, n, 40, [(n // 4, n // 2), (5 * n // 8, 7 * n // 8)], freq=300.0 + 150 * i, rate=rate)
            for i, n in enumerate(lens)]
    norm = feature_stats(sigs, rate)
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
    frames = b.lengths.tolist()
    b.close()
    return dict(sigs=sigs, norm=norm, dec=dec, ref_words=ref_words, ref=ref, frames=frames)


def ticks_of(sigs):
    for t in range(max(-(-len(s) // TICK) for s in sigs)):
        live = [k for k, s in enumerate(sigs) if t * TICK < len(s)]
        yield live, [sigs[k][t * TICK:(t + 1) * TICK] for k in live], [(t + 1) * TICK >= len(sigs[k]) for k in live]


def test_push_audio_decodes_like_the_one_shot_path(hip, ctx, e2e):
    from sr.feature import StreamingFrontend
    dec, sigs = e2e["dec"], e2e["sigs"]
    fe = StreamingFrontend(6, 16000, normalize=e2e["norm"], max_chunk=TICK)
    on = dec.online(6, max_frames=max(e2e["frames"]), frontend=fe)
    for ids, chunks, end in ticks_of(sigs):
        on.push_audio(ids, chunks, end)
    assert on.frames.tolist() == e2e["frames"] and fe.samples.tolist() == [len(s) for s in sigs]
    with pytest.raises(ValueError):
        on.push_audio([0], [sigs[0][:TICK]])                                # ended, and past max_frames
    words, info = on.result(np.arange(6))
    assert words == e2e["ref_words"] and all(len(w) >= 1 for w in words)
    np.testing.assert_array_equal(info["best_end"], e2e["ref"]["best_end"])
    np.testing.assert_allclose(info["end_cost"].reshape(-1), e2e["ref"]["end_cost_flat"], rtol=1e-12)
    on.finish([2])                                                          # frees the id in the front-end too
    assert fe.samples[2] == 0 and on.frames[2] == 0
    for ids, chunks, end in ticks_of([sigs[0]]):
        on.push_audio([2], chunks, end)
    words2, info2 = on.result([2])
    assert words2 == e2e["ref_words"][:1]
    np.testing.assert_allclose(info2["end_cost"][0], info["end_cost"][0], rtol=1e-12)
    on.close()
    fe.close()


def test_push_audio_with_a_window_settles_a_prefix(hip, ctx, e2e):
    from sr.feature import StreamingFrontend
    dec, sigs = e2e["dec"], e2e["sigs"]
    fe = StreamingFrontend(6, 16000, normalize=e2e["norm"], max_chunk=TICK)
    on = dec.online(6, window=max(e2e["frames"]) + 8, frontend=fe)
    seen = [[] for _ in sigs]
    for ids, chunks, end in ticks_of(sigs):
        on.push_audio(ids, chunks, end)
        for k, new in zip(ids, on.commit(ids)):
            seen[k] += new
            assert seen[k] == e2e["ref_words"][k][:len(seen[k])]            # settled words are a prefix of the final words
    words, info = on.result(np.arange(6))
    assert words == e2e["ref_words"]
    np.testing.assert_allclose(info["end_cost"].reshape(-1), e2e["ref"]["end_cost_flat"], rtol=1e-12)
    assert on.settled(np.arange(6))[0] == seen
    on.close()
    fe.close()
