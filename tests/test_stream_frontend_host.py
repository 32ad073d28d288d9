# -*- coding: utf-8 -*-
"""The streaming front-end on the host (no GPU).

1. `frames_ready` against the contract spelled out frame by frame (stream_frontend_ref.frames_ready_brute).
2. The carried stack (stream_frontend_ref.CarriedStack: 4 cepstral rows carried, rows arriving in arbitrary groups) against
   the oracle's stack of the whole matrix -- subtractions only, so BITWISE.
3. The host logic of `sr.feature.StreamingFrontend` and `OnlineDecoder.push_audio` on test doubles of the binding
   (tests/fake_hip.py, the `OnlineSession` double of test_online_settle_host.py, `FakeStreamFrontend`): refusals touch nothing, a
   `_room` refusal leaves both objects where they were, `finish` frees the id for a new utterance."""
import numpy as np
import pytest

import fake_hip
from oracle import ref_numpy as O
from stream_frontend_ref import CarriedStack, FakeStreamFrontend, frames_ready_brute, raw_stack
from test_online_settle_host import FakeSettleSession


@pytest.mark.parametrize("flen,step", [(400, 160), (200, 80), (7, 3)])
def test_frames_ready_against_brute_force(flen, step):
    from sr.recognition import _hip
    n = np.arange(3001)
    for ended in (False, True):
        got = _hip.stream_frames_ready(n, flen, step, ended)
        want = [frames_ready_brute(int(k), flen, step, ended) for k in n]
        np.testing.assert_array_equal(got, want)
    assert _hip.stream_frames_ready(flen + 3 * step, flen, step) == 2 and isinstance(_hip.stream_frames_ready(5, flen, step), int)
    # the closed form of the contract: C(n), P(n) = C & ~1, max(0, P - 2)
    c = np.where(n < flen, 0, (n - flen) // step + 1)
    np.testing.assert_array_equal(_hip.stream_frames_ready(n, flen, step), np.maximum((c & ~1) - 2, 0))


def test_frames_ready_of_the_package_uses_the_mfcc_geometry():
    from sr.feature import frames_ready
    assert frames_ready(399) == 0 and frames_ready(400 + 3 * 160) == 2 and frames_ready(161, ended=True) == 2
    assert frames_ready(3000, ended=True, sample_rate=8000) == 38          # step 80
    assert frames_ready(200 + 3 * 80, sample_rate=8000) == 2


@pytest.mark.parametrize("T", [2, 3, 4, 5, 26, 100])
def test_carried_stack_is_the_whole_stack_bitwise(T):
    rng = np.random.default_rng(100 + T)
    for trial in range(20):
        ceps = rng.normal(size=(T, 13)) * 10.0
        cuts = [0]
        while cuts[-1] < T:                                # groups of 0, 1 or a few rows
            cuts.append(min(T, cuts[-1] + int(rng.choice([0, 1, 1, 2, 3, 7]))))
        end_alone = bool(trial % 2)                        # the end flag on the last rows, or on an empty group of its own
        cs, out = CarriedStack(13), []
        for k in range(len(cuts) - 1):
            last = k == len(cuts) - 2
            out.append(cs.push(ceps[cuts[k]:cuts[k + 1]], end=last and not end_alone))
            if not (last and not end_alone):
                assert cs.done == max(0, cuts[k + 1] - 2)  # every row whose two successors exist, no other
        if end_alone:
            out.append(cs.push(ceps[:0], end=True))
        got = np.concatenate(out)
        np.testing.assert_array_equal(got, raw_stack(ceps))
        if T >= 3:                                         # (two frames have a constant delta track: std = 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                np.testing.assert_array_equal(O.standardize(got), O.stack_features(ceps))
    with pytest.raises(IndexError):
        CarriedStack(13).push(np.zeros((1, 13)), end=True)


# ------------------------------------------------------------------ host logic on the doubles
@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", FakeSettleSession, raising=False)
    monkeypatch.setattr(_hip, "StreamFrontend", FakeStreamFrontend, raising=False)
    monkeypatch.setattr(FakeSettleSession, "calls", 0)
    monkeypatch.setattr(FakeStreamFrontend, "pushes", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def pcm(rng, n):
    return (rng.normal(size=n) * 3000).astype(np.int16)


def test_streaming_frontend_is_chunking_invariant_on_the_double(fake_backend):
    """The double computes cepstra with the oracle, so this checks the bookkeeping: ids in any order, streams that sit a
    tick out, `frames_ready` per push, and the concatenated output = the whole utterance's stack."""
    from sr.feature import StreamingFrontend
    rng = np.random.default_rng(3)
    sigs = [pcm(rng, n) for n in (161, 800, 1700, 2500)]
    fe = StreamingFrontend(4, max_chunk=900)
    got, pos = [[] for _ in sigs], [0] * 4
    while any(pos[k] < len(sigs[k]) or not fe._ended[k] for k in range(4)):
        ids = [int(k) for k in rng.permutation(4) if not fe._ended[k]]
        lens = [int(min(rng.integers(0, 700), len(sigs[k]) - pos[k])) for k in ids]
        end = [pos[k] + c == len(sigs[k]) and rng.random() < 0.7 for k, c in zip(ids, lens)]
        before = fe.samples[ids]
        b = fe.push(ids, [sigs[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)], end)
        want = fe.frames_ready(before + np.array(lens), end) - fe.frames_ready(before)
        assert b.lengths.tolist() == list(want)
        for u, (k, c) in enumerate(zip(ids, lens)):
            got[k].append(b.features()[u])
            pos[k] += c
        assert fe.samples.tolist() == pos
    for k, s in enumerate(sigs):
        np.testing.assert_array_equal(np.concatenate(got[k]), raw_stack(O.mfcc_features_signal(s, 16000)[1]))


def test_streaming_frontend_refusals_touch_nothing(fake_backend):
    from sr.feature import StreamingFrontend
    rng = np.random.default_rng(4)
    fe = StreamingFrontend(3, max_chunk=500)
    x = pcm(rng, 300)
    fe.push([2, 0], [x, x[:100]])
    fe.push([1], [x], end=[True])
    before, calls = fe.samples, FakeStreamFrontend.pushes
    assert before.tolist() == [100, 300, 300] and calls == 2
    for ids, chunks, end in (([0, 0], [x, x], None),                       # an id twice
                             ([0, 3], [x, x], None), ([-1], [x], None),    # ids out of range
                             ([0, 2], [x, pcm(rng, 501)], None),           # a chunk over max_chunk: stream 0 must not move either
                             ([0, 1], [x, x], None),                       # audio after the end
                             ([0], [x.astype(np.float32)], None),          # not int16
                             ([0], [x.reshape(2, 150)], None),             # not one-dimensional
                             ([0, 2], [x], None),                          # chunks and ids do not pair up
                             ([0, 2], [x, x], [True]),                     # ... nor the end flags
                             ([0], [x[:60]], [True])):                     # 160 samples: one frame
        with pytest.raises(ValueError):
            fe.push(ids, chunks, end)
        assert fe.samples.tolist() == before.tolist() and FakeStreamFrontend.pushes == calls
    fresh = StreamingFrontend(1)
    with pytest.raises(ValueError):
        fresh.push([0], [x[:0]], [True])                                   # an end without a sample
    with pytest.raises(ValueError):
        fe.reset([3])
    fe.push([0], [x[:61]], [True])                                         # 161 samples: two frames, fine
    fe.reset([1])
    assert fe.samples.tolist() == [161, 0, 300]
    assert fe.push([1], [x]).lengths.tolist() == [0]                       # the id takes a new utterance
    with pytest.raises(ValueError):
        StreamingFrontend(2, normalize=(np.zeros(39), np.zeros(39)))       # std = 0
    with pytest.raises(ValueError):
        StreamingFrontend(2, normalize=(np.zeros(13), np.ones(13)))


W_, N_, M_ = 3, 3, 2


def make_decoder(rng, **kw):
    import sr.recognition as R
    from sr.recognition.batch import ContinuousDecoder
    from test_online_host import word_trans
    hmms = []
    for i in range(W_):
        h = R.HMM(N_)
        h.gmm_states = []
        for s in range(N_):
            mean, var = rng.normal(size=(M_, 39)) * 5.0, rng.uniform(20.0, 60.0, size=(M_, 39))
            g = R.GMM(mean[0].copy(), var[0].copy(), M_)
            g.update_models(mean, var, rng.dirichlet(np.ones(M_)))
            h.gmm_states.append(g)
        h.transitions = word_trans(rng, N_)
        hmms.append(h)
    return ContinuousDecoder(hmms, grammar="loop", word_penalty=0.3, **kw)


def test_push_audio_bookkeeping_and_refusals(fake_backend):
    from sr.feature import StreamingFrontend
    from sr.recognition import _hip
    rng = np.random.default_rng(5)
    dec = make_decoder(rng)
    with pytest.raises(ValueError):
        dec.online(2, max_frames=10, frontend=StreamingFrontend(3))        # another number of streams
    with pytest.raises(ValueError):
        dec.online(2, max_frames=10, frontend=StreamingFrontend(2, dtype=np.float32))
    with pytest.raises(ValueError):
        dec.online(2, max_frames=10).push_audio([0], [pcm(rng, 100)])     # no front-end
    fe = StreamingFrontend(2, max_chunk=4000)
    on = dec.online(2, max_frames=12, frontend=fe)
    sig = [pcm(rng, 2400), pcm(rng, 1700)]                                 # 15 and 11 frames
    on.push_audio([1, 0], [sig[1][:1000], sig[0][:1200]])                  # 2 and 4 frames
    assert fe.samples.tolist() == [1200, 1000] and on.frames.tolist() == [4, 2]
    on.push_audio([0], [sig[0][1200:1300]])                                # nothing final: the decoder is not called
    assert on.frames.tolist() == [4, 2] and FakeSettleSession.calls == 1 and FakeStreamFrontend.pushes == 2
    state = (fe.samples.tolist(), on.frames.tolist(), FakeSettleSession.calls, FakeStreamFrontend.pushes)
    for ids, chunks, end in (([0, 1], [sig[0][1300:], sig[1][1000:]], [True, True]),   # stream 0: 15 frames > 12 -- stream 1 stays too
                             ([1, 1], [sig[1][:10], sig[1][:10]], None),
                             ([1], [sig[1][1000:].astype(np.int32)], None),
                             ([2], [sig[1][:10]], None)):
        with pytest.raises(ValueError):
            on.push_audio(ids, chunks, end)
        assert (fe.samples.tolist(), on.frames.tolist(), FakeSettleSession.calls, FakeStreamFrontend.pushes) == state
    on.push_audio([1], [sig[1][1000:]], end=[True])
    assert on.frames.tolist() == [4, 11]
    with pytest.raises(ValueError):
        on.push_audio([1], [sig[1][:10]])                                  # the utterance has ended
    # the result is the decode of the whole utterance's features; finish frees the id in both objects
    b = _hip.Batch(dec.ctx, [raw_stack(O.mfcc_features_signal(sig[1], 16000)[1])])
    want = dec.decode_batch(b)
    words, info = on.finish([1])
    assert words == want[0]
    np.testing.assert_array_equal(info["end_cost"].reshape(-1), want[1]["end_cost_flat"])
    assert on.frames.tolist() == [4, 0] and fe.samples.tolist() == [1300, 0]
    on.push_audio([1], [sig[0][:1200]])                                    # a new utterance on the freed id
    assert on.frames.tolist() == [4, 4] and fe.samples.tolist() == [1300, 1200]
    on.reset()
    assert on.frames.tolist() == [0, 0] and fe.samples.tolist() == [0, 0]
    # push / push_batch keep working on a decoder with a front-end
    on.push([0], [rng.normal(size=(3, 39))])
    assert on.frames.tolist() == [3, 0] and fe.samples.tolist() == [0, 0]


def test_push_audio_window_refusal_moves_neither_object(fake_backend):
    from sr.feature import StreamingFrontend
    rng = np.random.default_rng(6)
    dec = make_decoder(rng)
    fe = StreamingFrontend(1, max_chunk=4000)
    on = dec.online(1, window=5, frontend=fe)
    sig = pcm(rng, 3000)
    on.push_audio([0], [sig[:1200]])                                       # 4 frames
    with pytest.raises(ValueError):
        on.push_audio([0], [sig[1200:2000]])                               # 4 more: 8 unsettled > 5
    assert fe.samples.tolist() == [1200] and on.frames.tolist() == [4]
