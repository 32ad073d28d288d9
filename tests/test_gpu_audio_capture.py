# -*- coding: utf-8 -*-
"""sr.audio_capture on the GPU: batched endpoint detection (csrc/gh_endpoint.hip) against G21 -- the reference's own
AudioRecorder.record_callback -- and against the numpy restatement (tests/audio_capture_ref.py, pinned to the reference
by tests/test_audio_capture_host.py), and the endpointed MFCC front-end against host-side trimming.

Decisions (indices, segment counts, per-frame attributes) must be EXACT; level / background / energy agree to 1e-10
absolute, the project's fp64 tolerance: the device's energies differ from numpy's by a few ulp of ~100 dB (log10 is the
one operation whose rounding may differ), about 3e-14; the level is a convex combination of energies and the background
a damped one, so neither amplifies that."""
import wave

import numpy as np
import pytest

import audio_capture_ref as A
from conftest import load_golden
from test_audio_capture_host import g21_cases

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def AC():
    import sr.audio_capture as AC
    return AC


@pytest.fixture(scope="module")
def ctx():
    from sr.recognition import _hip
    return _hip.default_context()


def burst_signal(rng, n, sigma, bursts, amp=4000.0, freq=440.0, rate=8000):
    t = np.arange(n) / rate
    x = rng.normal(0.0, sigma, size=n) if sigma > 0 else np.zeros(n)
    for a, b in bursts:
        x[a:b] += amp * np.sin(2 * np.pi * freq * t[a:b])
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def three_bursts():
    """The issue's example: 6 s at 8 kHz, sigma 50, a 440 Hz tone of amplitude 4000 over three ranges."""
    return burst_signal(np.random.default_rng(0), 48000, 50, [(8000, 13000), (22000, 27000), (36000, 41000)])


def same_as_restatement(res, u, ref, max_segments):
    k = len(ref["start"])
    assert int(res["n_segments"][u]) == len(ref["end"]) == k, (u, res["n_segments"][u], ref["start"], ref["end"])
    assert bool(res["open"][u]) == ref["open"], u
    assert res["start"][u, :k].tolist() == ref["start"] and res["end"][u, :k].tolist() == ref["end"], u
    assert not res["start"][u, k:].any() and not res["end"][u, k:].any(), u
    assert int(res["frames_done"][u]) == ref["frames_done"], u
    assert k <= max_segments


# ------------------------------------------------------------------ 5: G21
def test_detect_endpoints_reproduces_the_reference(AC):
    g = load_golden("G21_endpoints")
    for ci in range(2):
        cases = [c for c in g21_cases(g) if int(g["config_of"][c[0]]) == ci]
        raw = cases[0][3]
        for cfg in (dict(raw), dict(cases[0][4])):        # as the user writes it, and already derived
            res = AC.detect_endpoints([c[2] for c in cases], cfg, want_frames=True)
            for u, (si, pp, x, _, der) in enumerate(cases):
                has, is_open = bool(res["n_segments"][u]), bool(res["open"][u])
                assert (int(res["start"][u, 0]) if has else 0) == int(g[pp + "start"]), si
                assert (int(res["end"][u, 0]) if has and not is_open else 0) == int(g[pp + "end"]), si
                assert is_open == bool(g[pp + "started"]), si
                if is_open:
                    assert int(res["end"][u, 0]) == len(x) - 1
                nfr = len(g[pp + "is_speech"])
                assert int(res["frames_done"][u]) == nfr, si
                assert len(res["is_speech"][u]) == A.frame_count(len(x), der['samples per frame'], der['frame stride'])
                np.testing.assert_array_equal(res["is_speech"][u][:nfr], g[pp + "is_speech"])
                for mine, ref in ((res["level"][u][:nfr], g[pp + "level"]), (res["energy"][u][:nfr], g[pp + "energy"]),
                                  (res["background"][u][10:nfr], g[pp + "backgrounds"]),
                                  (res["level"][u][10:nfr], g[pp + "levels"])):
                    err = float(np.max(np.abs(mine - ref))) if len(ref) else 0.0
                    print("G21 s%d: max abs error %.3g" % (si, err))
                    assert err <= TOL, (si, err)
                for k in ("is_speech", "level", "background", "energy"):      # nothing behind the frame it stopped at
                    assert not np.any(res[k][u][nfr:]), (si, k)
        assert raw == cases[0][3]                          # derived on a copy


# ------------------------------------------------------------------ 6: seeded sweep
SWEEP = [
    ("default 8 kHz", dict(A.DEFAULT_CONFIG), 1),
    ("16 kHz, 400 / 160 samples, forget factor 100",
     dict(A.DEFAULT_CONFIG, **{'sample rate': 16000, 'forget factor': 100, 'frame time': 0.025, 'frame stride': 0.01,
                               'adjustment': 0.02, 'onset threshold': 4, 'offset threshold': 0.5,
                               'silence threshold': 300, 'speech threshold': 100, 'start boundary': 100}), 4),
    ("8 kHz, 240 / 80 samples, forget factor 5",
     dict(A.DEFAULT_CONFIG, **{'forget factor': 5, 'frame time': 0.03, 'adjustment': 0.05, 'onset threshold': 2.5,
                               'offset threshold': 1.0, 'silence threshold': 200, 'speech threshold': 60}), 2),
    ("11025 Hz, 220 / 110 samples (gcd not a multiple of 8)",
     dict(A.DEFAULT_CONFIG, **{'sample rate': 11025, 'forget factor': 2, 'silence threshold': 250,
                               'speech threshold': 120}), 3),
]


@pytest.mark.parametrize("name,raw,max_segments", SWEEP, ids=[s[0] for s in SWEEP])
def test_seeded_sweep_against_the_restatement(AC, name, raw, max_segments):
    n_rec = 2000
    rng = np.random.default_rng(600 + max_segments)
    rate = raw['sample rate']
    cfg = A.derive(raw)
    sigs = []
    for i in range(n_rec):
        kind = i % 10
        n = int(rng.integers(0, 3 * cfg['samples per frame'])) if kind == 0 else int(rng.integers(0, int(3.5 * rate)))
        bursts = []
        for _ in range(int(rng.integers(0, 4))):
            if n > 10:
                a = int(rng.integers(0, n))
                bursts.append((a, min(n, a + int(rng.integers(rate // 20, rate)))))
        sigma = 0.0 if kind == 1 else float(rng.uniform(0.3, 300))
        sigs.append(burst_signal(rng, n, sigma, bursts, amp=float(rng.uniform(200, 12000)), freq=float(rng.uniform(100, 2000)),
                                 rate=rate))
    sigs[3] = np.zeros(0, dtype=np.int16)
    sigs[5] = burst_signal(rng, 2 * rate, 50, [(rate // 2, rate)], amp=400000.0, rate=rate)   # clipped to full scale: the largest sums
    res = AC.detect_endpoints(sigs, dict(raw), max_segments=max_segments, want_frames=True)
    left_out = n_segs = n_open = n_carried = 0
    for u, x in enumerate(sigs):
        ref = A.detect(x, cfg, max_segments)
        if ref["margin"] < 1e-9:
            left_out += 1
            continue
        same_as_restatement(res, u, ref, max_segments)
        np.testing.assert_array_equal(res["is_speech"][u], ref["is_speech"])      # the frames' ATTRIBUTE, every frame
        n_carried += int(ref["clamped_while_carrying"])
        n_segs += len(ref["start"])
        n_open += ref["open"]
    print("%s: %d recordings, %d segments (%d open), %d left out" % (name, n_rec, n_segs, n_open, left_out))
    assert left_out <= n_rec // 100
    assert n_segs >= n_rec // 4 and n_open >= 10                  # the sweep does exercise the detector
    print("%s: %d frames in the clamp branch while a speech decision was carried" % (name, n_carried))
    assert n_carried >= 100                                       # ... and the branch where attribute and decision part ways


def test_per_frame_outputs_against_the_restatement(AC):
    rng = np.random.default_rng(77)
    raw = SWEEP[1][1]
    cfg = A.derive(raw)
    sigs = [burst_signal(rng, int(rng.integers(0, 40000)), float(rng.uniform(1, 200)),
                         [(int(a), int(a) + 6000) for a in rng.integers(0, 30000, size=2)], rate=16000) for _ in range(64)]
    res = AC.detect_endpoints(sigs, dict(raw), max_segments=3, want_frames=True)
    worst = 0.0
    for u, x in enumerate(sigs):
        ref = A.detect(x, cfg, 3)
        same_as_restatement(res, u, ref, 3)
        np.testing.assert_array_equal(res["is_speech"][u], ref["is_speech"])
        for k in ("level", "background", "energy"):
            assert res[k][u].shape == ref[k].shape
            if len(ref[k]):
                worst = max(worst, float(np.max(np.abs(res[k][u] - ref[k]))))
    print("per-frame level / background / energy: max abs error %.3g" % worst)
    assert worst <= TOL


# ------------------------------------------------------------------ 7: max_segments
def test_max_segments_on_three_bursts(AC):
    x = three_bursts()
    cfg = A.derive(A.DEFAULT_CONFIG)
    want = [(9920, 17280), (23920, 31280), (37920, 45280)]
    others = [burst_signal(np.random.default_rng(s), 40000, 30, [(5000, 9000), (17000, 21000), (29000, 34000)]) for s in (1, 2)]
    sigs = [x, x[:39000]] + others
    first = None
    for m in (1, 2, 8):
        res = AC.detect_endpoints(sigs, max_segments=m)
        assert res["start"].shape == res["end"].shape == (len(sigs), m)
        for u, s in enumerate(sigs):
            same_as_restatement(res, u, A.detect(s, cfg, m), m)
        k = min(m, 3)
        assert list(zip(res["start"][0, :k].tolist(), res["end"][0, :k].tolist())) == want[:k]
        assert int(res["n_segments"][0]) == k and not res["open"][0]         # the cap stops detection
        if m == 1:
            first = res
        np.testing.assert_array_equal(res["start"][:, 0], first["start"][:, 0])
        np.testing.assert_array_equal(res["end"][:, 0], first["end"][:, 0])
    assert res["start"][1].tolist()[:3] == [9920, 23920, 37920] and res["end"][1].tolist()[:3] == [17280, 31280, 38999]
    assert int(res["n_segments"][1]) == 3 and res["open"][1]                 # two segments and an open third


# ------------------------------------------------------------------ 8: chunks
def test_chunked_call_equals_the_one_chunk_call(AC, ctx, monkeypatch):
    rng = np.random.default_rng(8)
    sigs = [burst_signal(rng, int(rng.integers(6000, 30000)), 40, [(3000, 7000), (12000, 16000)]) for _ in range(40)]
    monkeypatch.delenv("GMMHMM_SCRATCH_BUDGET", raising=False)
    one = AC.detect_endpoints(sigs, max_segments=2, want_frames=True)
    assert ctx.last_chunks == 1
    monkeypatch.setenv("GMMHMM_SCRATCH_BUDGET", "256K")
    many = AC.detect_endpoints(sigs, max_segments=2, want_frames=True)
    assert ctx.last_chunks >= 3
    monkeypatch.delenv("GMMHMM_SCRATCH_BUDGET")
    assert one["n_segments"].sum() >= 40
    for k in ("start", "end", "n_segments", "open", "frames_done", "frame_off"):
        np.testing.assert_array_equal(one[k], many[k])
    for k in ("is_speech", "level", "background", "energy"):
        for a, b in zip(one[k], many[k]):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 9: endpointed front-end
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("max_segments", [1, 3])
def test_endpointed_features_equal_host_trimming(AC, dtype, max_segments):
    from sr.feature import features_from_signals
    rng = np.random.default_rng(9)
    rate = 16000
    sigs = [burst_signal(rng, int(rng.integers(20000, 90000)), float(rng.uniform(5, 80)),
                         [(int(a), int(a) + int(rng.integers(6000, 12000))) for a in rng.integers(3000, 70000, size=3)],
                         rate=rate) for _ in range(12)]
    sigs += [burst_signal(rng, 100000, s, [(10000, 18000), (40000, 48000), (70000, 78000)], rate=rate) for s in (20, 60)]
    sigs.append(burst_signal(rng, 9000, 30, [], rate=rate))                  # no segment: stays whole
    sigs.append(burst_signal(rng, 30000, 30, [(15000, 30000)], rate=rate))   # open
    for cfg in (True, dict(SWEEP[1][1])):
        b = features_from_signals(sigs, rate, dtype=dtype, endpoints=cfg, max_segments=max_segments)
        raw = AC.default_config(rate) if cfg is True else cfg
        det = AC.detect_endpoints(sigs, dict(raw), max_segments=max_segments)
        for k in ("start", "end", "n_segments", "open"):
            np.testing.assert_array_equal(b.endpoints[k], det[k])
        begin, stop = AC.trim_ranges(det, [len(x) for x in sigs], dict(raw))
        rec = np.repeat(np.arange(len(sigs)), np.maximum(det["n_segments"], 1))
        np.testing.assert_array_equal(b.endpoints["recording"], rec)
        assert det["n_segments"].max() == max_segments and (det["n_segments"] == 0).any() and det["open"].any()
        host = features_from_signals([sigs[r][a:e] for r, a, e in zip(rec, begin, stop)], rate, dtype=dtype)
        assert b.U == host.U == len(rec)
        np.testing.assert_array_equal(b.offsets, host.offsets)
        got, want = b.features(), host.features()
        for a, e in zip(got, want):
            assert a.dtype == e.dtype == np.dtype(dtype)
            np.testing.assert_array_equal(a, e)                              # same kernel, same samples: bit for bit
        b.close()
        host.close()


# ------------------------------------------------------------------ 10: AudioRecorder.process
def test_audio_recorder_process_against_the_reference(AC, tmp_path):
    from scipy.io import wavfile
    g = load_golden("G21_endpoints")
    for si, pp, x, raw, der in g21_cases(g):
        ar = AC.AudioRecorder(dict(raw))
        assert ar.process(x) is ar
        assert ar.speech_start_index == int(g[pp + "start"]) and ar.speech_end_index == int(g[pp + "end"]), si
        assert ar.started_speech == bool(g[pp + "started"]), si
        assert len(ar.samples) == int(g[pp + "n_fed"]), si           # what the reference's callback was handed
        assert ar.samples == x[:len(ar.samples)].tolist()
        for k in ("levels", "backgrounds", "final_levels"):
            assert len(getattr(ar, k)) == len(g[pp + k]), (si, k)
            if len(g[pp + k]):
                assert np.max(np.abs(np.array(getattr(ar, k)) - g[pp + k])) <= TOL, (si, k)
        got = ar.get_samples()
        s0 = max(int(g[pp + "start"]) - der['start boundary'], 0)
        assert got.dtype == np.int16 and len(got) == int(g[pp + "n_get_samples"]), si
        np.testing.assert_array_equal(got, x[s0:s0 + len(got)])
        assert ar.frames == []
        if len(got):
            path = str(tmp_path / ("s%d.wav" % si))
            ar.write_to_wav_file(path)
            rate, back = wavfile.read(path)
            assert rate == der['sample rate']
            np.testing.assert_array_equal(back, got)
            with wave.open(path, "rb") as wf:
                assert (wf.getnchannels(), wf.getsampwidth(), wf.getnframes()) == (1, 2, len(got))


# ------------------------------------------------------------------ 11: end to end
def test_raw_recordings_to_decoded_words(AC, ctx):
    import sr.recognition as R
    from sr.feature import features_from_signals
    from sr.recognition.batch import ContinuousDecoder, IsolatedWordRecognizer
    from test_gpu_api import make_hmm
    rng = np.random.default_rng(11)
    rate = 16000
    sigs = [burst_signal(rng, 40000, 40, [(12000, 22000)], freq=300.0 + 150 * i, rate=rate) for i in range(5)]
    sigs.append(burst_signal(rng, 80000, 40, [(12000, 22000), (45000, 56000)], rate=rate))
    b = features_from_signals(sigs, rate, endpoints=True, max_segments=2)
    det = b.endpoints
    assert det["n_segments"].tolist() == [1, 1, 1, 1, 1, 2] and b.U == 7
    begin, stop = AC.trim_ranges(det, [len(x) for x in sigs], AC.default_config(rate))
    assert np.all(begin > 0) and np.all(stop < np.array([len(sigs[r]) for r in det["recording"]]))   # noise on both sides is cut
    frames = [ctx.lib.gh_mfcc_frames(int(n), rate, 0.01) for n in stop - begin]
    assert b.lengths.tolist() == frames and b.D == 39
    W, n, M, D = 3, 4, 2, 39
    trans = np.full((n, n), np.inf)
    for i in range(n):
        trans[i, i] = -np.log(0.8) if i < n - 1 else 0.0
        if i < n - 1:
            trans[i + 1, i] = -np.log(0.2)
    hmms = [make_hmm(R, rng.normal(size=(n, M, D)), rng.uniform(0.5, 1.5, size=(n, M, D)), rng.dirichlet(np.ones(M), size=n), trans)
            for _ in range(W)]
    gmm = IsolatedWordRecognizer(hmms, ctx=ctx)
    nll = b.loglik(gmm.gmm)
    assert nll.shape == (b.N, W * n) and np.all(np.isfinite(nll))
    costs = gmm.costs(b)
    assert costs.shape == (b.U, W) and np.all(np.isfinite(costs))
    words, _ = ContinuousDecoder(hmms, grammar="loop", ctx=ctx).decode_batch(b)
    assert len(words) == b.U and all(len(w) >= 1 for w in words)
    b.close()
