# -*- coding: utf-8 -*-
"""Streaming endpoint detection on the host (no GPU).

1. The carried detector restated in numpy (stream_endpoints_ref.carried_step) against `audio_capture_ref.detect` of the whole
   recording with a large `max_segments`: equal starts, ends and `open`, `array_equal` per-frame arrays, for the recordings
   and cuttings the GPU test uses.
2. Frames after n samples and the carry bound against brute force; width % stride != 0 is a ValueError.
3. The host logic of `StreamingEndpointer`, its gate and `OnlineDecoder.push_recording` on test doubles of the binding, with
   the restatement as the backend: every utterance's (begin, stop) equals `get_samples_range` of the offline detection."""
import numpy as np
import pytest

import audio_capture_ref as A
import fake_hip
import stream_endpoints_ref as S
from stream_frontend_ref import FakeStreamFrontend
from test_online_settle_host import FakeSettleSession

LARGE = 1000


# ------------------------------------------------------------------ 1: the restatement
@pytest.mark.parametrize("name,raw", S.CONFIGS, ids=[c[0] for c in S.CONFIGS])
def test_carried_detector_equals_detect_for_every_cutting(name, raw):
    cfg = A.derive(raw)
    width, stride = cfg['samples per frame'], cfg['frame stride']
    sigs, _ = S.recordings(raw, 40)
    rng = np.random.default_rng(41)
    n_seg = n_open = 0
    for index, x in enumerate(sigs):
        ref = A.detect(x, cfg, max_segments=LARGE)
        n_seg += len(ref["start"])
        n_open += ref["open"]
        for how, lengths in S.cuttings(rng, len(x), width, stride, index).items():
            events, frames, st, longest = S.feed(x, cfg, lengths)
            starts, ends, is_open = S.segments_of(events)
            assert (starts, ends, is_open) == (ref["start"], ref["end"], ref["open"]), (index, how)
            assert st["frames"] == ref["frames_done"] == A.frame_count(len(x), width, stride), (index, how)
            assert longest < 2 * width - stride
            for k in ("is_speech", "level", "background", "energy"):
                np.testing.assert_array_equal(frames[k], ref[k], err_msg="%s of recording %d, %s" % (k, index, how))
    assert n_seg >= 10 and n_open >= 1


# ------------------------------------------------------------------ 2: frames and the carry
@pytest.mark.parametrize("width,stride", [(160, 80), (240, 80), (220, 110), (320, 160)])
def test_frames_and_carry_against_brute_force(width, stride, monkeypatch, built_library):
    from sr.recognition import _hip
    from sr.audio_capture import StreamingEndpointer
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "EndpointStream", S.FakeEndpointStream, raising=False)
    cfg = dict(A.derive(A.DEFAULT_CONFIG), **{'samples per frame': width, 'frame stride': stride})
    ep = StreamingEndpointer(1, cfg)
    n = np.arange(5 * width + 1)
    want = [S.frames_brute(int(k), width, stride) for k in n]
    assert want == [A.frame_count(int(k), width, stride) for k in n]
    np.testing.assert_array_equal(ep.frames_after(n), want)
    carry = [S.carry_brute(int(k), width, stride) for k in n]
    np.testing.assert_array_equal(ep.carry_after(n), carry)
    assert 0 <= min(carry) and max(carry) == 2 * width - stride - 1 < ep.carry_cap == 2 * width - stride
    assert isinstance(ep.frames_after(width), int) and ep.frames_after(2 * width) == 1 + width // stride


@pytest.mark.parametrize("width,stride", [(400, 160), (7, 3), (1323, 441 * 2)])
def test_a_framing_that_falls_behind_is_refused(width, stride):
    from sr.audio_capture import StreamingEndpointer
    cfg = dict(A.derive(A.DEFAULT_CONFIG), **{'samples per frame': width, 'frame stride': stride})
    with pytest.raises(ValueError, match="detect_endpoints"):
        StreamingEndpointer(2, cfg)                        # (before any context is made: this runs without a GPU)
    # ... and why: without divisibility the carry grows with every chunk
    grow = [S.carry_brute(c * width, width, stride) for c in range(1, 40)]
    assert grow[-1] - grow[0] == 38 * (width - int(width / stride) * stride) > 0
    with pytest.raises(ValueError):
        StreamingEndpointer(0)
    with pytest.raises(ValueError):
        StreamingEndpointer(1, max_chunk=0)


# ------------------------------------------------------------------ 3: host logic on the doubles
@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", FakeSettleSession, raising=False)
    monkeypatch.setattr(_hip, "StreamFrontend", FakeStreamFrontend, raising=False)
    monkeypatch.setattr(_hip, "EndpointStream", S.FakeEndpointStream, raising=False)
    monkeypatch.setattr(FakeSettleSession, "calls", 0)
    monkeypatch.setattr(FakeStreamFrontend, "pushes", 0)
    monkeypatch.setattr(S.FakeEndpointStream, "pushes", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def offline_ranges(x, cfg):
    ref = A.detect(x, cfg, max_segments=LARGE)
    return [A.get_samples_range(s, e, len(x), cfg['start boundary']) if not (ref["open"] and j == len(ref["end"]) - 1)
            else (max(s - cfg['start boundary'], 0), len(x)) for j, (s, e) in enumerate(zip(ref["start"], ref["end"]))], ref


def run_gate(ep, k, x, lengths, end_alone=False):
    """Feed x to stream k through the gate; returns the utterances [(begin, stop, open, samples)] the rounds carry."""
    utts, open_piece, pos = [], [], 0
    plan = [(c, j == len(lengths) - 1 and not end_alone) for j, c in enumerate(lengths)] + ([(0, True)] if end_alone or not lengths else [])
    for c, fin in plan:
        rounds = ep.gate([k], [x[pos:pos + c]], [fin])
        pos += c
        for ids, pieces, flags, ranges in rounds:
            assert ids.tolist() == [k] and len(pieces) == len(flags) == len(ranges) == 1
            assert pieces[0].dtype == np.int16 and len(pieces[0]) <= ep.max_piece
            open_piece.append(pieces[0])
            assert (ranges[0] is not None) == bool(flags[0])
            if flags[0]:
                utts.append(ranges[0] + (np.concatenate(open_piece),))
                open_piece = []
    assert not open_piece                                  # the end of the recording closes what is open
    return utts


@pytest.mark.parametrize("name,raw", S.CONFIGS[:2] + S.CONFIGS[3:], ids=[c[0] for c in S.CONFIGS[:2] + S.CONFIGS[3:]])
def test_gate_hands_out_the_offline_ranges_for_every_cutting(fake_backend, name, raw):
    from sr.audio_capture import StreamingEndpointer
    cfg = A.derive(raw)
    width, stride = cfg['samples per frame'], cfg['frame stride']
    sigs, _ = S.recordings(raw, 40)
    rng = np.random.default_rng(42)
    ep = StreamingEndpointer(3, dict(raw), max_chunk=int(3.5 * raw['sample rate']))
    n_utt = n_open = 0
    for index, x in enumerate(sigs):
        want, ref = offline_ranges(x, cfg)
        for how, lengths in S.cuttings(rng, len(x), width, stride, index).items():
            if how == "one":
                continue                                   # (the restatement has had this cutting; the gate gets its own below)
            ep.reset([1])
            got = run_gate(ep, 1, x, lengths, end_alone=bool(index % 2))
            assert [(b, e) for b, e, _, _ in got] == want, (index, how)
            assert [o for _, _, o, _ in got] == [False] * (len(want) - 1) + [ref["open"]] * bool(want), (index, how)
            for b, e, _, samples in got:
                np.testing.assert_array_equal(samples, x[b:e])
        n_utt += len(want)
        n_open += ref["open"]
    assert n_utt >= 10 and n_open >= 1


def test_gate_end_sample_that_arrives_late_or_never(fake_backend):
    """The end frame is the last frame of the last chunk: speech_end_index = i stride + width = n, one past the newest sample."""
    from sr.audio_capture import StreamingEndpointer
    cfg = A.derive(A.DEFAULT_CONFIG)
    width = cfg['samples per frame']
    x = S.burst_signal(np.random.default_rng(0), 48000, 50, [(8000, 13000), (22000, 27000), (36000, 41000)])
    want, _ = offline_ranges(x, cfg)
    assert want == [(9920 - 1600, 17281), (23920 - 1600, 31281), (37920 - 1600, 45281)]
    ep = StreamingEndpointer(2, max_chunk=48000)
    # the recording is cut right behind the first end frame: 17280 = 108 chunks of 160
    assert 17280 % width == 0
    r1 = ep.gate([0], [x[:17280]])
    assert [len(p[0]) for _, p, _, _ in r1] == [17280 - 8320] and not r1[0][2][0]      # forwarded, still open: sample 17280 is missing
    assert ep.gate([0], [x[:0]]) == []                                                # a tick without audio: still waiting
    r2 = ep.gate([0], [x[17280:20000]])
    assert len(r2) == 1 and len(r2[0][1][0]) == 1 and r2[0][2][0] and r2[0][3][0] == (8320, 17281, False)
    # ... or never: the recording ends there, and the utterance is clipped to n like trim_ranges' min(end + 1, n)
    ep.reset([0])
    r1 = ep.gate([0], [x[:17280]], [True])
    assert len(r1) == 1 and r1[0][3][0] == (8320, 17280, False) and len(r1[0][1][0]) == 17280 - 8320
    assert A.get_samples_range(9920, 17280, 17280, 1600) == (8320, 17280)
    # ... also when the end flag comes on an empty push of its own
    ep.reset([0])
    ep.gate([0], [x[:17280]])
    r2 = ep.gate([0], [x[:0]], [True])
    assert len(r2) == 1 and len(r2[0][1][0]) == 0 and r2[0][2][0] and r2[0][3][0] == (8320, 17280, False)


def test_gate_two_events_of_one_stream_give_two_rounds(fake_backend):
    from sr.audio_capture import StreamingEndpointer
    x = S.burst_signal(np.random.default_rng(0), 48000, 50, [(8000, 13000), (22000, 27000), (36000, 41000)])
    y = S.burst_signal(np.random.default_rng(1), 30000, 50, [(8000, 13000)])
    ep = StreamingEndpointer(3, max_chunk=48000)
    rounds = ep.gate([2, 0], [x, y], [True, False])        # three utterances of stream 2, one of stream 0, in one push
    assert [r[0].tolist() for r in rounds] == [[2, 0], [2], [2]]
    assert [r[3][0] for r in rounds] == [(8320, 17281, False), (22320, 31281, False), (36320, 45281, False)]
    assert rounds[0][3][1][2] is False and all(len(set(r[0].tolist())) == len(r[0]) for r in rounds)
    for r in rounds:
        for k, piece, flag, rg in zip(*r):
            np.testing.assert_array_equal(piece, (x if k == 2 else y)[rg[0]:rg[1]])
    # an end and the next start in one push: the first round ends an utterance, the second opens one
    ep.reset()
    ep.gate([1], [x[:12000]])
    rounds = ep.gate([1], [x[12000:26000]])
    assert [(r[2].tolist(), r[3]) for r in rounds] == [([True], [(8320, 17281, False)]), ([False], [None])]
    np.testing.assert_array_equal(rounds[1][1][0], x[22320:26000])


def test_refused_push_moves_nothing_and_reset_clears_the_lookback(fake_backend):
    from sr.audio_capture import StreamingEndpointer
    rng = np.random.default_rng(4)
    x = S.burst_signal(rng, 12000, 50, [(3000, 9000)])
    ep = StreamingEndpointer(3, max_chunk=6000)
    ep.gate([2, 0], [x[:6000], x[:100]])
    ep.push([1], [x[:300]], end=[True])
    before, calls = ep.samples, S.FakeEndpointStream.pushes
    kept = [k.copy() for k in ep._keep]
    assert before.tolist() == [100, 300, 6000] and calls == 2
    for call in (ep.push, ep.gate):
        for ids, chunks, end in (([0, 0], [x[:10], x[:10]], None),                     # an id twice
                                 ([0, 3], [x[:10], x[:10]], None), ([-1], [x[:10]], None),   # ids out of range
                                 ([0, 2], [x[:10], x[:6001]], None),                   # a chunk over max_chunk: stream 0 must not move either
                                 ([0, 1], [x[:10], x[:10]], None),                     # audio after the end
                                 ([0], [x[:10].astype(np.float32)], None),             # not int16
                                 ([0], [x[:10].reshape(2, 5)], None),                  # not one-dimensional
                                 ([0, 2], [x[:10]], None),                             # chunks and ids do not pair up
                                 ([0, 2], [x[:10], x[:10]], [True])):                  # ... nor the end flags
            with pytest.raises(ValueError):
                call(ids, chunks, end)
            assert ep.samples.tolist() == before.tolist() and S.FakeEndpointStream.pushes == calls
            assert all(np.array_equal(a, b) for a, b in zip(kept, ep._keep))
    with pytest.raises(ValueError):
        ep.reset([3])
    # stream 2 is inside an utterance; a reset forgets it and the id reproduces a fresh recording
    assert ep._utt[2] is not None and len(ep._keep[2])
    ep.reset([2])
    assert ep._utt[2] is None and len(ep._keep[2]) == 0 and ep.samples.tolist() == [100, 300, 0]
    got = run_gate(ep, 2, x, [6000, 6000])
    fresh = StreamingEndpointer(1, max_chunk=6000)
    assert [g[:3] for g in got] == [g[:3] for g in run_gate(fresh, 0, x, [6000, 6000])] and len(got) == 1
    ep.reset()
    assert ep.samples.tolist() == [0, 0, 0]


# ------------------------------------------------------------------ push_recording on the doubles
def test_push_recording_bookkeeping_and_refusals(fake_backend):
    from sr.audio_capture import StreamingEndpointer
    from sr.feature import StreamingFrontend
    from sr.recognition import _hip
    from oracle import ref_numpy as O
    from stream_frontend_ref import raw_stack
    from test_stream_frontend_host import make_decoder
    rng = np.random.default_rng(5)
    dec = make_decoder(rng)
    raw = dict(A.DEFAULT_CONFIG, **{'sample rate': 16000, 'silence threshold': 100, 'speech threshold': 50, 'start boundary': 20})
    cfg = A.derive(raw)
    ep = StreamingEndpointer(2, dict(raw), max_chunk=1600)
    assert ep.max_piece == 320 + 480 + 1600 and ep.min_utterance == 320 + 320
    with pytest.raises(ValueError):
        dec.online(2, max_frames=100, endpointer=ep)                                   # no front-end
    with pytest.raises(ValueError):
        dec.online(2, max_frames=100, frontend=StreamingFrontend(2, max_chunk=ep.max_piece - 1), endpointer=ep)
    with pytest.raises(ValueError):
        dec.online(2, max_frames=100, frontend=StreamingFrontend(2, 8000, max_chunk=4000), endpointer=ep)     # another sample rate
    with pytest.raises(ValueError):
        dec.online(2, max_frames=100, frontend=StreamingFrontend(2, max_chunk=4000), endpointer=StreamingEndpointer(3, dict(raw)))
    short = dict(raw, **{'frame time': 0.005, 'frame stride': 0.005, 'start boundary': 0})                # utterances of 80 samples
    with pytest.raises(ValueError):
        dec.online(2, max_frames=100, frontend=StreamingFrontend(2, max_chunk=40000), endpointer=StreamingEndpointer(2, short))
    with pytest.raises(ValueError):
        dec.online(2, max_frames=100, frontend=StreamingFrontend(2, max_chunk=4000)).push_recording([0], [np.zeros(10, dtype=np.int16)])
    fe = StreamingFrontend(2, max_chunk=ep.max_piece)
    on = dec.online(2, max_frames=60, frontend=fe, endpointer=ep)
    x = S.burst_signal(rng, 16000, 40, [(3000, 6000), (10000, 13000)], rate=16000)
    want, ref = offline_ranges(x, cfg)
    assert len(want) == 2 and not ref["open"]
    got = []
    for t in range(0, 16000, 1600):
        got += on.push_recording([1], [x[t:t + 1600]], [t + 1600 >= 16000])
    assert [(u["stream"], u["begin"], u["stop"], u["open"]) for u in got] == [(1, b, e, False) for b, e in want]
    for u in got:                                           # the words are the decode of that slice alone
        b = _hip.Batch(dec.ctx, [raw_stack(O.mfcc_features_signal(x[u["begin"]:u["stop"]], 16000)[1])])
        assert u["words"] == dec.decode_batch(b)[0][0]
    assert on.frames.tolist() == [0, 0] and fe.samples.tolist() == [0, 0] and ep.samples.tolist() == [0, 16000]
    # bad arguments: nothing moves in any of the three objects
    state = (ep.samples.tolist(), fe.samples.tolist(), on.frames.tolist(), S.FakeEndpointStream.pushes)
    for ids, chunks, end in (([0, 0], [x[:10], x[:10]], None), ([1], [x[:10]], None), ([0], [x[:1601]], None), ([2], [x[:10]], None)):
        with pytest.raises(ValueError):
            on.push_recording(ids, chunks, end)
        assert (ep.samples.tolist(), fe.samples.tolist(), on.frames.tolist(), S.FakeEndpointStream.pushes) == state
    # an utterance longer than max_frames: the decoder refuses, the endpointer has moved, the streams are named, reset frees them
    long_one = S.burst_signal(rng, 16000, 40, [(3000, 15000)], rate=16000)
    with pytest.raises(ValueError, match=r"streams \[0\].*reset"):
        for t in range(0, 16000, 1600):
            on.push_recording([0], [long_one[t:t + 1600]])
    assert ep.samples[0] > 0
    on.reset([0])
    assert ep.samples.tolist() == [0, 16000] and fe.samples.tolist() == [0, 0] and on.frames.tolist() == [0, 0]
    got = []
    for t in range(0, 16000, 1600):
        got += on.push_recording([0], [x[t:t + 1600]], [t + 1600 >= 16000])
    assert [(u["begin"], u["stop"]) for u in got] == want
    on.reset()
    assert ep.samples.tolist() == [0, 0]
