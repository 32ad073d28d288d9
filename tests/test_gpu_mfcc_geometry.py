# -*- coding: utf-8 -*-
"""The MFCC front-end (csrc/gh_mfcc.hip, gh_mfcc_core.h, gh_mfcc_stream.hip) at every geometry, on silent frames and at
every position in a batch.

The reference is tests/mfcc_ref.py, the extended-precision restatement of `mfcc_features` with a direct DFT, pinned by
test_mfcc_ref_host.py (which also asserts what is assumed here about the inputs: frame counts, silent rows).  Tolerances
are the ones this kernel is held to elsewhere and no other: rtol = atol = 1e-9 for filterbank and cepstra
(test_gpu_kernels.py), 1e-7 for fp64 and 2e-5 for fp32 stacked features (test_mfcc_at_scale_matches_oracle), bitwise
where two paths of the project are compared with each other.

Everything a frame's result depends on besides its own samples is covered: the window padding and the mel table (1, 2, 6,
7), the end of the utterance (2), and the frame's partner in the wave -- two frames share one complex FFT -- when the
partner is silent, when the frame itself is (3), when one is 1e9 times the other's power (4), and which frame that is (5:
frames pair inside their utterance, so an utterance is bitwise the same alone, anywhere in a batch, and streamed: 9)."""
import ctypes as C

import numpy as np
import pytest

import mfcc_ref as M
from stream_frontend_ref import raw_stack
from test_gpu_stream_frontend import cut, stream_all

pytestmark = pytest.mark.gpu

TOL = 1e-9
SWEEP = M.GEOMETRIES + [M.DEFAULT]


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


_REF = {}


def ref_of(key, signal, geo):
    """The reference of a signal at a geometry, computed once and shared (never written to)."""
    if key not in _REF:
        fb, mf = M.mfcc_features_ref(signal, geo[1], *M.params(geo))
        fb.setflags(write=False)
        mf.setflags(write=False)
        _REF[key] = (fb, mf)
    return _REF[key]


def check(got_fb, got_mf, ref, what):
    fb, mf = ref
    assert got_fb.shape == fb.shape and got_mf.shape == mf.shape, what
    print("%s: fbank %.3g cepstra %.3g" % (what, np.max(np.abs(got_fb - fb) / (1 + np.abs(fb))), np.max(np.abs(got_mf - mf) / (1 + np.abs(mf)))))
    np.testing.assert_allclose(got_fb, fb, rtol=TOL, atol=TOL, err_msg=what + " fbank")
    np.testing.assert_allclose(got_mf, mf, rtol=TOL, atol=TOL, err_msg=what + " cepstra")


def mode1(hip, ctx, sigs, geo=M.DEFAULT, dtype=np.float64, **kw):
    """The raw [ceps | delta | delta-delta] rows of every utterance through the resident front-end."""
    b = hip.Batch(ctx, pcm=sigs, sample_rate=geo[1], mfcc_params=M.params(geo), frontend_mode=1, dtype=dtype, **kw)
    try:
        return [f.copy() for f in b.features()]
    finally:
        b.close()


# ------------------------------------------------------------------ 1: geometry sweep
@pytest.mark.parametrize("geo", SWEEP, ids=lambda g: g[0])
def test_geometry_sweep(hip, ctx, geo):
    sigs = M.sweep_signals(geo)
    fbs, mfs = hip.mfcc(ctx, sigs, geo[1], M.params(geo))
    refs = [ref_of(("sweep", geo[0], u), x, geo) for u, x in enumerate(sigs)]
    for u in range(len(sigs)):
        check(fbs[u], mfs[u], refs[u], "%s utterance %d" % (geo[0], u))
    if geo[0] == "80-400":                                 # the empty filters: log10(eps) in every frame, exactly
        empty = np.all(refs[0][0] == M.LOG_EPS, axis=0)
        assert empty.any()
        for fb in fbs:
            np.testing.assert_array_equal(fb[:, empty], M.LOG_EPS)
    # the resident chain on the same batch: 39 stacked columns in both dtypes
    for dt, tol in ((np.float64, 1e-7), (np.float32, 2e-5)):
        for u, f in enumerate(mode1(hip, ctx, sigs, geo, dt)):
            np.testing.assert_allclose(f, raw_stack(refs[u][1]), rtol=tol, atol=tol, err_msg="%s stacked %d" % (geo[0], u))


# ------------------------------------------------------------------ 2: length edges
@pytest.mark.parametrize("geo", [M.DEFAULT, M.GEOMETRIES[0], M.GEOMETRIES[2]], ids=lambda g: g[0])
def test_length_edges(hip, ctx, geo):
    sigs = M.edge_signals(geo)
    fbs, mfs = hip.mfcc(ctx, sigs, geo[1], M.params(geo))
    assert [len(fb) for fb in fbs] == [M.frame_count(len(x), geo[7]) for x in sigs]
    for u, x in enumerate(sigs):
        ref = ref_of(("edge", geo[0], u), x, geo)
        check(fbs[u], mfs[u], ref, "%s %d samples in the batch" % (geo[0], len(x)))
        fb1, mf1 = hip.mfcc(ctx, [x], geo[1], M.params(geo))
        check(fb1[0], mf1[0], ref, "%s %d samples alone" % (geo[0], len(x)))
        np.testing.assert_array_equal(fb1[0], fbs[u])
        np.testing.assert_array_equal(mf1[0], mfs[u])


# ------------------------------------------------------------------ 3: silent frames
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_silent_frames(hip, ctx, case):
    """A frame without a non-zero sample is the reference's log10(eps) row whatever shares its FFT.  (Case b has one silent
    frame per utterance by construction -- an A beside a loud B in the first, a B beside a loud A in the second.)"""
    from sr.feature import StreamingFrontend
    sigs = M.silent_cases()[case]
    refs = [ref_of(("silent", case, u), x, M.DEFAULT) for u, x in enumerate(sigs)]
    quiet = [M.silent_rows(r[0]) for r in refs]
    slots = {int(t) % 2 for q in quiet for t in np.flatnonzero(q)}
    assert slots == {0, 1}                                 # a silent row in an A slot and one in a B slot
    fbs, mfs = hip.mfcc(ctx, sigs, 16000)
    for u in range(len(sigs)):
        if quiet[u].any():
            print("case %s utterance %d: silent rows %s, log filterbank there %.6g .. %.6g" %
                  (case, u, np.flatnonzero(quiet[u]).tolist(), fbs[u][quiet[u]].min(), fbs[u][quiet[u]].max()))
        check(fbs[u], mfs[u], refs[u], "silence %s utterance %d" % (case, u))
        np.testing.assert_array_equal(fbs[u][quiet[u]], M.LOG_EPS)
    # the resident front-end, and a stream cut in 37-sample chunks: the silent rows' 13 raw cepstra
    got = mode1(hip, ctx, sigs)
    fe = StreamingFrontend(len(sigs), 16000, max_chunk=37)
    rng = np.random.default_rng(3)
    streamed = stream_all(fe, rng, sigs, [cut(rng, len(x), 37) for x in sigs], [False] * len(sigs))
    fe.close()
    for u in range(len(sigs)):
        for f, what in ((got[u], "batch"), (streamed[u], "stream")):
            np.testing.assert_allclose(f[quiet[u], :13], refs[u][1][quiet[u]], rtol=1e-7, atol=1e-7, err_msg="%s %s %d" % (what, case, u))
            np.testing.assert_allclose(f, raw_stack(refs[u][1]), rtol=1e-7, atol=1e-7, err_msg="%s %s %d" % (what, case, u))


# ------------------------------------------------------------------ 4: quiet beside loud
def test_quiet_frames_beside_loud_ones(hip, ctx):
    """Frames of +-1 LSB share their FFT with full-scale ones (256 / 256: no overlap).  The partner's leakage is some
    2.5e-16 of the loud spectrum in amplitude, about 4e-12 relative on the quiet frame's power: this is the bound that
    makes packing two frames into one transform acceptable, and 1e-9 holds it with a margin in the hundreds."""
    geo = M.GEOMETRIES[2]
    sigs = M.quiet_loud_signals()
    fbs, mfs = hip.mfcc(ctx, sigs, geo[1], M.params(geo))
    for u, x in enumerate(sigs):
        check(fbs[u], mfs[u], ref_of(("quietloud", u), x, geo), "quiet beside loud, %s first" % ("loud", "quiet")[u])


# ------------------------------------------------------------------ 5: batch position
def test_batch_position_bitwise(hip, ctx):
    """Utterances of 3, 26, 5 and 12 frames: each is bit for bit what it is alone, in this order and in reverse."""
    from sr.audio_capture.record import _derived
    sigs = M.position_signals()
    cfg = _derived(None, 16000)
    entries = {
        "gh_mfcc fbank": lambda s: hip.mfcc(ctx, s, 16000)[0],
        "gh_mfcc cepstra": lambda s: hip.mfcc(ctx, s, 16000)[1],
        "batch fp64": lambda s: mode1(hip, ctx, s, dtype=np.float64),
        "batch fp32": lambda s: mode1(hip, ctx, s, dtype=np.float32),
        "endpointed fp64": lambda s: mode1(hip, ctx, s, dtype=np.float64, endpoints=cfg),
        "endpointed fp32": lambda s: mode1(hip, ctx, s, dtype=np.float32, endpoints=cfg),
    }
    for name, run in entries.items():
        alone = [run([x])[0] for x in sigs]
        assert [len(a) for a in alone] == [3, 26, 5, 12], name         # (no recording is cut by the endpoint detector)
        for order in (range(4), range(3, -1, -1)):
            together = run([sigs[u] for u in order])
            for u, f in zip(order, together):
                np.testing.assert_array_equal(f, alone[u], err_msg="%s: utterance %d in the order %s" % (name, u, list(order)))


# ------------------------------------------------------------------ 6: closed-form spectra
@pytest.mark.parametrize("case", ["impulse at 700", "impulse at 860", "alternating", "constant"])
def test_closed_form_spectra(hip, ctx, case):
    """No transform on the reference side: the filterbank against log10(power @ fbank.T) of the closed form."""
    geo = M.GEOMETRIES[0]
    x, power = M.closed_form_cases()[case]
    ref = M.finish(power, geo[1], geo[4], geo[5])
    fbs, mfs = hip.mfcc(ctx, [x], geo[1], M.params(geo))
    check(fbs[0], mfs[0], ref, case)
    quiet = M.silent_rows(ref[0])
    np.testing.assert_array_equal(fbs[0][quiet], M.LOG_EPS)
    if case == "alternating":                              # bin 256: lane 0, register 4
        assert np.all(np.argmax(power, axis=1) == 256)


# ------------------------------------------------------------------ 7: formats
def test_sample_formats(hip, ctx):
    geo = M.GEOMETRIES[3]                                  # 11 025 Hz: 275 / 110, padded to 512
    rng = np.random.default_rng(7)
    x = M.chirp_noise(rng, 2345, geo[1])
    ref = ref_of(("formats", "int"), x, geo)
    for dt in (np.int16, np.float32, np.float64):          # (the three are not bit-equal to each other: profiles/mfcc_core_kernel_times.txt)
        fbs, mfs = hip.mfcc(ctx, [x.astype(dt)], geo[1], M.params(geo))
        check(fbs[0], mfs[0], ref, "integer-valued signal as %s" % np.dtype(dt).name)
    y = rng.uniform(-1, 1, size=2345)
    fbs, mfs = hip.mfcc(ctx, [y], geo[1], M.params(geo))
    check(fbs[0], mfs[0], ref_of(("formats", "f64"), y, geo), "float64 in [-1, 1]")
    z = rng.uniform(-1, 1, size=2345).astype(np.float32)   # float32 is widened to fp64 before pre-emphasis
    assert np.any(z != np.round(z))
    f32 = hip.mfcc(ctx, [z], geo[1], M.params(geo))
    f64 = hip.mfcc(ctx, [z.astype(np.float64)], geo[1], M.params(geo))
    rz = ref_of(("formats", "f32"), z.astype(np.float64), geo)
    check(f32[0][0], f32[1][0], rz, "float32 in [-1, 1]")
    check(f64[0][0], f64[1][0], rz, "its float64 copy")
    np.testing.assert_allclose(f32[0][0], f64[0][0], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(f32[1][0], f64[1][0], rtol=TOL, atol=TOL)


# ------------------------------------------------------------------ 8: refusals
def raw_mfcc(hip, ctx, rate, prm, samples, s_off, f_off, fb, mf):
    s_off, f_off = np.asarray(s_off, dtype=np.int64), np.asarray(f_off, dtype=np.int64)
    fs, st, lo, hi = prm
    hip._check(ctx.lib, ctx.lib.gh_mfcc(ctx.h, 0, int(rate), float(fs), float(st), float(lo), 0.0 if hi is None else float(hi),
                                        len(s_off) - 1, samples.ctypes.data_as(C.c_void_p), hip._ptr(s_off, hip._c_i64p),
                                        hip._ptr(f_off, hip._c_i64p), hip._ptr(fb, hip._c_f64p), hip._ptr(mf, hip._c_f64p)))


def test_refusals(hip, ctx):
    x = M.chirp_noise(np.random.default_rng(8), 1600, 16000)
    default = (0.025, 0.01, 80, None)
    cases = [
        ("a mel point on bin 258", (0.025, 0.01, 80, 8050), [0, 1600], [0, 10]),
        ("a frame of 513 samples", (513.5 / 16000, 0.01, 80, None), [0, 1600], [0, 10]),
        ("a step below one sample", (0.025, 1e-5, 80, None), [0, 1600], [0, 10]),
        ("frame_off one frame short", default, [0, 800, 1600], [0, 5, 9]),
        ("an empty utterance", default, [0, 0, 1600], [0, 0, 10]),
    ]
    for what, prm, s_off, f_off in cases:
        fb, mf = np.full((10, 40), np.nan), np.full((10, 13), np.nan)
        with pytest.raises(hip.BackendError):
            raw_mfcc(hip, ctx, 16000, prm, x, s_off, f_off, fb, mf)
        assert np.isnan(fb).all() and np.isnan(mf).all(), what         # nothing was computed
    fb, mf = np.full((10, 40), np.nan), np.full((10, 13), np.nan)      # the same call goes through when nothing is wrong
    raw_mfcc(hip, ctx, 16000, default, x, [0, 800, 1600], [0, 5, 10], fb, mf)
    check(fb[:5], mf[:5], ref_of(("refusal", 0), x[:800], M.DEFAULT), "the accepted call")
    # the Python entries refuse the same inputs
    for prm in (cases[0][1], cases[1][1]):
        with pytest.raises(hip.BackendError):
            hip.mfcc(ctx, [x], 16000, prm)
        with pytest.raises(hip.BackendError):
            hip.Batch(ctx, pcm=[x], sample_rate=16000, mfcc_params=prm, frontend_mode=1)
        with pytest.raises(hip.BackendError):
            hip.StreamFrontend(ctx, 1, 16000, prm)


# ------------------------------------------------------------------ 9: streaming at every geometry
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("geo", SWEEP, ids=lambda g: g[0])
def test_streams_at_every_geometry_bitwise(hip, ctx, geo, dtype):
    """One utterance cut three ways (whole, 37-sample chunks, seeded random with empty chunks) in three streams of one
    front-end: each is bit for bit the one-shot front-end of the utterance alone; `stream_all` checks `frames_ready` at
    every push."""
    from sr.feature import StreamingFrontend
    name, rate, fs, st, lo, hi = geo[:6]
    x = M.sweep_signals(geo)[2]                            # 3 001 samples
    want = mode1(hip, ctx, [x], geo, dtype)[0]
    rng = np.random.default_rng(9)
    plans = [cut(rng, len(x), how) for how in ("whole", 37, "random")]
    while 0 not in plans[2]:                               # (a fifth of the random chunks are empty)
        plans[2] = cut(rng, len(x), "random")
    fe = StreamingFrontend(3, rate, max_chunk=len(x), dtype=dtype, frame_size=fs, frame_stride=st, low_freq=lo, high_freq=hi)
    got = stream_all(fe, rng, [x, x, x], plans, [False, True, True])
    fe.close()
    for f, how in zip(got, ("whole", "37-sample chunks", "random chunks")):
        assert f.dtype == dtype
        np.testing.assert_array_equal(f, want, err_msg="%s, %s" % (name, how))
    if dtype == np.float64:
        np.testing.assert_allclose(want, raw_stack(ref_of(("sweep", name, 2), x, geo)[1]), rtol=1e-7, atol=1e-7)
