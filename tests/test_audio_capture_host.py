# -*- coding: utf-8 -*-
"""sr.audio_capture without a GPU: the numpy restatement of the reference's endpoint detection (tests/audio_capture_ref.py)
against G21 -- what the reference's own AudioRecorder.record_callback computed --, the distance of every G21 frame from
the thresholds it is compared with (what makes exact decisions a fair demand of the device), the package's host side
(import without pyaudio, config derivation, input errors before any library call) and trim_ranges."""
import sys

import numpy as np
import pytest

import audio_capture_ref as A
from conftest import load_golden

INT_KEYS = ('samples per frame', 'frame stride', 'silence threshold', 'speech threshold', 'start boundary', 'end boundary',
            'sample rate', 'channel count', 'chunk size')


def g21_configs(g):
    """(raw, derived) dicts of G21's two configs."""
    out = []
    for ci in range(2):
        raw = dict(zip([str(k) for k in g["config_keys"]], g["c%d_raw" % ci]))
        der = dict(zip([str(k) for k in g["derived_keys"]], g["c%d_derived" % ci]))
        for d, ints in ((raw, INT_KEYS[6:]), (der, INT_KEYS)):
            for k in ints:
                d[k] = int(d[k])
            d['format'] = 8
        out.append((raw, der))
    return out


def g21_cases(g):
    cfgs = g21_configs(g)
    for si in range(int(g["n_signals"])):
        ci = int(g["config_of"][si])
        yield si, "s%d_" % si, g["s%d_x" % si], cfgs[ci][0], cfgs[ci][1]


def test_restatement_reproduces_the_reference():
    g = load_golden("G21_endpoints")
    seen_open = seen_closed = seen_none = 0
    for si, pp, x, raw, der in g21_cases(g):
        d = A.derive(raw)
        for k in der:
            if k != 'format':
                assert d[k] == der[k], (si, k)
        r = A.detect(x, der)
        start = r["start"][0] if r["start"] else 0
        end = r["end"][0] if r["end"] and not r["open"] else 0
        assert start == int(g[pp + "start"]) and end == int(g[pp + "end"]), si
        assert r["open"] == bool(g[pp + "started"]), si
        nfr = len(g[pp + "is_speech"])          # frames the reference appended: up to the one at which it stopped
        assert r["frames_done"] == nfr, si
        assert A.frame_count(len(x), der['samples per frame'], der['frame stride']) >= nfr
        np.testing.assert_array_equal(r["is_speech"][:nfr], g[pp + "is_speech"])
        for k in ("levels", "backgrounds", "final_levels"):
            assert len(r[k]) == len(g[pp + k]) == max(nfr - 10, 0), (si, k)
            np.testing.assert_allclose(r[k], g[pp + k], rtol=0, atol=1e-12)
        np.testing.assert_allclose(r["level"][:nfr], g[pp + "level"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(r["energy"][:nfr], g[pp + "energy"], rtol=0, atol=1e-12)
        b, e = A.get_samples_range(start, end, int(g[pp + "n_fed"]), der['start boundary'])
        assert max(e - b, 0) == int(g[pp + "n_get_samples"]), si
        seen_open += r["open"]
        seen_closed += bool(r["end"]) and not r["open"]
        seen_none += not r["start"]
    assert seen_open >= 2 and seen_closed >= 4 and seen_none >= 3


def test_golden_frames_keep_their_distance_from_the_thresholds():
    g = load_golden("G21_endpoints")
    for si, pp, x, raw, der in g21_cases(g):
        r = A.detect(x, der)
        assert r["margin"] >= 1e-9, (si, r["margin"])


def test_issue_example_three_bursts():
    rng = np.random.default_rng(0)
    t = np.arange(48000) / 8000
    x = rng.normal(0, 50, 48000)
    for a, b in ((8000, 13000), (22000, 27000), (36000, 41000)):
        x[a:b] += 4000 * np.sin(2 * np.pi * 440 * t[a:b])
    x = np.round(x).astype(np.int16)
    cfg = A.derive(A.DEFAULT_CONFIG)
    r = A.detect(x, cfg, 8)
    assert list(zip(r["start"], r["end"])) == [(9920, 17280), (23920, 31280), (37920, 45280)] and not r["open"]
    assert list(zip(*[A.detect(x, cfg, 1)[k] for k in ("start", "end")])) == [(9920, 17280)]
    r = A.detect(x[:39000], cfg, 8)
    assert list(zip(r["start"], r["end"])) == [(9920, 17280), (23920, 31280), (37920, 38999)] and r["open"]


def test_import_without_pyaudio_and_config_derivation(tmp_path):
    assert "pyaudio" not in sys.modules
    import sr.audio_capture as AC
    assert "pyaudio" not in sys.modules
    for name in ("decode_audio_stream", "AudioFrame", "AudioRecorder", "record", "detect_endpoints", "trim_ranges"):
        assert hasattr(AC, name)
    assert AC.decode_audio_stream(np.array([1, -2, 3], dtype=np.int16).tobytes()) == [1, -2, 3]
    f = AC.AudioFrame([100, -200, 300])
    assert f.calc_energy() == 10 * np.log10(140000) and AC.AudioFrame([1, 0]).calc_energy() == 0
    ar = AC.AudioRecorder()
    want = A.derive(A.DEFAULT_CONFIG)
    assert ar.config == want
    g = load_golden("G21_endpoints")
    raw, der = g21_configs(g)[1]
    mine = dict(raw)
    ar = AC.AudioRecorder(mine)
    assert ar.config is mine                      # the reference writes the derived values back into the caller's dict
    assert mine == der
    assert (ar.speech_start_index, ar.speech_end_index, ar.started_speech) == (0, 0, False)
    assert ar.levels == ar.backgrounds == ar.final_levels == ar.frames == ar.samples == []
    with pytest.raises(ImportError, match="pyaudio"):
        ar.start_recording()
    with pytest.raises(ImportError, match="pyaudio"):
        AC.record(str(tmp_path / "a" / "x.wav"))


def test_input_errors_come_before_any_library_call(monkeypatch):
    import sr.audio_capture as AC
    from sr.recognition import _hip
    import sr.feature as F

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_hip, "default_context", boom)
    monkeypatch.setattr(_hip, "load_library", boom)
    ok = np.zeros(4000, dtype=np.int16)
    with pytest.raises(TypeError):
        AC.detect_endpoints([ok.astype(np.float32)])
    with pytest.raises(TypeError):
        AC.detect_endpoints([ok.astype(np.int32)])
    with pytest.raises(ValueError):
        AC.detect_endpoints([ok.reshape(2, -1)])
    with pytest.raises(ValueError):
        AC.detect_endpoints([ok], max_segments=0)
    with pytest.raises(ValueError):                                   # width < 1
        AC.detect_endpoints([ok], dict(A.DEFAULT_CONFIG, **{'frame time': 0.0001, 'frame stride': 0.0001}))
    with pytest.raises(ValueError):                                   # stride < 1
        AC.detect_endpoints([ok], dict(A.DEFAULT_CONFIG, **{'frame stride': 0.0001}))
    with pytest.raises(ValueError):                                   # stride > width
        AC.detect_endpoints([ok], dict(A.DEFAULT_CONFIG, **{'frame stride': 0.03}))
    with pytest.raises(ValueError, match="1280"):                     # 1323 / 441 samples, odd gcd: more units than fit LDS
        AC.detect_endpoints([ok], dict(A.DEFAULT_CONFIG, **{'sample rate': 44100, 'frame time': 0.03}))
    for k in ('sample rate', 'forget factor', 'frame time', 'frame stride', 'adjustment', 'onset threshold',
              'offset threshold', 'silence threshold', 'speech threshold', 'start boundary', 'end boundary'):
        cfg = dict(A.DEFAULT_CONFIG)
        del cfg[k]
        with pytest.raises(KeyError):
            AC.detect_endpoints([ok], cfg)
        if k in ('forget factor', 'adjustment', 'onset threshold', 'offset threshold'):
            with pytest.raises(KeyError):          # like the reference: __init__ does not look at them, classify_frame does
                AC.AudioRecorder(dict(cfg)).process(ok)
        else:
            with pytest.raises(KeyError):
                AC.AudioRecorder(dict(cfg))
    with pytest.raises(TypeError):
        AC.AudioRecorder().process(ok.astype(np.float64))
    with pytest.raises(ValueError, match="Hz"):
        F.features_from_signals([ok], sample_rate=16000, endpoints=dict(A.DEFAULT_CONFIG))
    with pytest.raises(TypeError):
        F.features_from_signals([ok.astype(np.float32)], endpoints=True)
    with pytest.raises(ValueError):
        F.features_from_signals([ok], endpoints=True, max_segments=0)
    user = dict(A.DEFAULT_CONFIG)
    with pytest.raises(AssertionError, match="library was reached"):    # valid input: the next step IS the library
        AC.detect_endpoints([ok, np.zeros(0, dtype=np.int16), np.zeros(50, dtype=np.int16)], user)
    assert user == A.DEFAULT_CONFIG                                   # detect_endpoints derives on a copy


def test_trim_ranges_on_hand_made_results():
    import sr.audio_capture as AC
    cfg = dict(A.DEFAULT_CONFIG)                     # start boundary 200 ms at 8 kHz = 1600 samples
    lengths = [12000, 12000, 5000, 9000, 20000]
    res = dict(start=np.array([[4880, 0], [800, 0], [0, 0], [3000, 0], [2000, 9000]]),
               end=np.array([[10880, 0], [11999, 0], [0, 0], [8999, 0], [6000, 19999]]),
               n_segments=np.array([1, 1, 0, 1, 2]), open=np.array([False, False, False, True, True]))
    begin, stop = AC.trim_ranges(res, lengths, cfg)
    #            ordinary      clipped at 0 and at the end   no segment: whole   open: to the end   closed + open
    assert begin.tolist() == [3280, 0, 0, 1400, 400, 7400]
    assert stop.tolist() == [10881, 12000, 5000, 9000, 6001, 20000]
    # end + 1 past the last sample (a segment that ends with the last whole chunk) is clipped
    res1 = dict(start=np.array([[4000]]), end=np.array([[12000]]), n_segments=np.array([1]), open=np.array([False]))
    assert [v.tolist() for v in AC.trim_ranges(res1, [12000], cfg)] == [[2400], [12000]]
    # an AudioRecorder's (derived) config means the same
    assert [v.tolist() for v in AC.trim_ranges(res1, [12000], AC.AudioRecorder().config)] == [[2400], [12000]]
    b0, s0 = AC.trim_ranges(dict(start=np.zeros((0, 1)), end=np.zeros((0, 1)), n_segments=np.zeros(0), open=np.zeros(0)), [], cfg)
    assert len(b0) == len(s0) == 0
