# -*- coding: utf-8 -*-
"""Extended-precision restatement of the reference's `mfcc_features` (sr/feature/feature.py:43-82) for the tests, and
the inputs the MFCC geometry tests share (numpy only, no GPU).

`mfcc_features_ref` follows feature.py line by line in `np.longdouble` (64-bit mantissa on x86: eps 1.1e-19).  The
spectrum is a direct 257 x 512 DFT, a matrix product with longdouble twiddles, not an FFT; the window, the mel points,
the triangles and the DCT are built here and share nothing with oracle/ref_numpy.py.  Where `np.longdouble` is no wider
than fp64 (`np.finfo(np.longdouble).eps` not below 1e-18) the same text computes in fp64 and every assertion stays.

Two places follow the reference's fp64 VALUE rather than a wider one, because the reference takes a discontinuous function
of it: the mel points go through `floor` (feature.py:64), so they are evaluated in the reference's own fp64 arithmetic,
and the test `filter_banks == 0` (:77) picks the fp64 eps.  Pre-emphasis uses the fp64 constant 0.97.

Where `final_len < len(signal)` (frames shorter than the step) the reference itself raises at `np.zeros(negative)`
(feature.py:17); like the oracle this restatement takes `max(0, ...)` there: the frames are cut from the signal as it
is.  A mel point past bin 257 raises IndexError like the reference's `fbank[m - 1, k]`."""
import functools

import numpy as np

LD = np.longdouble
NFFT, NFILT, NCEPS = 512, 40, 13
EPS = np.finfo(float).eps
LOG_EPS = float(np.log10(EPS))                             # what an all-zero frame, or an empty filter, comes out as
PI = 4 * np.arctan(LD(1))


def frame_geometry(sample_rate, frame_size, frame_stride):
    """(frame, step) in samples, feature.py:9-10."""
    return int(frame_size * sample_rate), int(frame_stride * sample_rate)


def frame_count(n, step):
    """feature.py:11-13: `slen > frame_len` compares samples with SECONDS and is always true."""
    return -(-n // step)


def pre_emphasis(signal):
    """feature.py:45-46."""
    x = np.asarray(signal).astype(LD)
    return np.append(x[0], x[1:] - LD(0.97) * x[:-1])


def hamming(M):
    """np.hamming: 0.54 - 0.46 cos(2 pi n / (M - 1)); ones for M == 1."""
    if M == 1:
        return np.ones(1, dtype=LD)
    return LD(0.54) - LD(0.46) * np.cos(2 * PI * np.arange(M).astype(LD) / (M - 1))


@functools.lru_cache(maxsize=None)
def dft_matrices():
    """cos / -sin of 2 pi k n / 512 for n in [0, 512), k in [0, 257): the angle is reduced exactly in integers first."""
    m = (np.arange(NFFT)[:, None] * np.arange(NFFT // 2 + 1)[None, :]) % NFFT
    ang = 2 * PI * m.astype(LD) / NFFT
    return np.cos(ang), -np.sin(ang)


def mel_bins(sample_rate, low_freq, high_freq):
    """feature.py:59-64 in the reference's fp64: the 42 bin points."""
    high_freq = high_freq or sample_rate / 2
    low_mel = 2595 * np.log10(1 + low_freq / 700)
    high_mel = 2595 * np.log10(1 + high_freq / 700)
    mel_points = np.linspace(low_mel, high_mel, NFILT + 2)
    hz_points = 700 * (10 ** (mel_points / 2595) - 1)
    return np.floor((NFFT + 1) * hz_points / sample_rate)


def mel_filterbank(sample_rate, low_freq=80, high_freq=None):
    """feature.py:66-75: the 40 triangles [40, 257], weights in extended precision."""
    b = mel_bins(sample_rate, low_freq, high_freq).astype(LD)
    fbank = np.zeros((NFILT, NFFT // 2 + 1), dtype=LD)
    for m in range(1, NFILT + 1):
        lo, ce, hi = int(b[m - 1]), int(b[m]), int(b[m + 1])
        for k in range(lo, ce):
            fbank[m - 1, k] = (k - b[m - 1]) / (b[m] - b[m - 1])
        for k in range(ce, hi):
            fbank[m - 1, k] = (b[m + 1] - k) / (b[m + 1] - b[m])
    return fbank


def log_filterbank(power, fbank):
    """feature.py:76-78 on a power spectrum [T, 257]."""
    fb = np.dot(power, fbank.T)
    return np.log10(np.where(fb == 0, LD(EPS), fb))


def dct_rows():
    """Rows 1 .. 13 of scipy's ortho DCT-II over 40 points (feature.py:80-81): sqrt(2 / N) cos(pi k (2 n + 1) / (2 N))."""
    k = np.arange(1, NCEPS + 1).astype(LD)[:, None]
    n = np.arange(NFILT).astype(LD)[None, :]
    return np.sqrt(LD(2) / NFILT) * np.cos(PI * k * (2 * n + 1) / (2 * NFILT))


def windowed_frames(signal, sample_rate, frame_size, frame_stride):
    """feature.py:45-52: pre-emphasis, `segment`, `zero_padding`, Hamming over the padded width.  [T, width]."""
    emphasized = pre_emphasis(signal)
    flen, step = frame_geometry(sample_rate, frame_size, frame_stride)
    num_frames = frame_count(emphasized.size, step)
    final_len = (num_frames - 1) * step + flen
    pad_sig = np.concatenate([emphasized, np.zeros(max(0, final_len - emphasized.size), dtype=LD)])
    frames = np.stack([pad_sig[i * step:i * step + flen] for i in range(num_frames)])
    width = 1 << (flen - 1).bit_length()
    left = (width - flen) // 2
    padded = np.zeros((num_frames, width), dtype=LD)
    padded[:, left:left + flen] = frames
    return padded * hamming(width)


def finish(power, sample_rate, low_freq, high_freq):
    """Power spectrum [T, 257] -> (log filterbank, cepstra) in fp64."""
    fb = log_filterbank(power, mel_filterbank(sample_rate, low_freq, high_freq))
    return fb.astype(np.float64), np.dot(fb, dct_rows().T).astype(np.float64)


def mfcc_features_ref(signal, sample_rate, frame_size=0.025, frame_stride=0.01, low_freq=80, high_freq=None):
    """(filter_banks [T, 40], mfcc [T, 13]) of an in-memory signal, rounded to fp64."""
    frames = windowed_frames(signal, sample_rate, frame_size, frame_stride)
    if frames.shape[1] > NFFT:                             # np.fft.rfft(frames, 512) would crop: the project refuses instead
        raise ValueError("frames of %d samples exceed NFFT" % frames.shape[1])
    c, s = dft_matrices()
    re, im = np.dot(frames, c[:frames.shape[1]]), np.dot(frames, s[:frames.shape[1]])
    power = (re * re + im * im) / NFFT
    return finish(power, sample_rate, low_freq, high_freq)


def silent_rows(fbank):
    """Rows of a log filterbank [T, 40] that are log10(eps) throughout: the frames without a non-zero sample."""
    return np.all(fbank == LOG_EPS, axis=1)


# ------------------------------------------------------------------ the inputs of the geometry tests
# name, rate, frame_size, frame_stride, low_freq, high_freq, frame and step in samples
GEOMETRIES = [
    ("512/160", 16000, 0.032, 0.01, 80, None, 512, 160),           # no padding at all
    ("257/160", 16000, 0.0160625, 0.01, 80, None, 257, 160),       # padded to 512 with an odd pad, pad_left 127
    ("256/256", 16000, 0.016, 0.016, 80, None, 256, 256),          # no overlap, window of 256 inside the 512-point FFT
    ("11025", 11025, 0.025, 0.01, 80, None, 275, 110),             # both products truncated
    ("22050", 22050, 0.02, 0.01, 80, None, 441, 220),
    ("44100", 44100, 0.01, 0.005, 80, None, 441, 220),             # mel point 0 falls on bin 0
    ("80/160", 16000, 0.005, 0.01, 80, None, 80, 160),             # gaps between frames
    ("2/160", 16000, 0.000125, 0.01, 80, None, 2, 160),            # hamming(2)
    ("1/16", 16000, 6.25e-5, 0.001, 80, None, 1, 16),              # the pad_w == 1 window
    ("low0", 16000, 0.025, 0.01, 0, None, 400, 160),
    ("300-3400", 16000, 0.025, 0.01, 300, 3400, 400, 160),
    ("80-1000", 16000, 0.025, 0.01, 80, 1000, 400, 160),           # 11 zero-width mel segments: filters of one zero weight
    ("80-400", 16000, 0.025, 0.01, 80, 400, 400, 160),             # 42 mel points on bins 2..12: empty filters
    ("80-8016", 16000, 0.025, 0.01, 80, 8016, 400, 160),           # the last mel point lands on bin 257
]
DEFAULT = ("default", 16000, 0.025, 0.01, 80, None, 400, 160)
SWEEP_LENGTHS = (1500, 2222, 3001, 3777, 4000)             # five ragged utterances per geometry


def params(geo):
    """The `mfcc_params` tuple of a geometry."""
    return geo[2:6]


def chirp_noise(rng, n, rate):
    """A chirp plus noise as int16: every bin carries energy."""
    t = np.arange(n) / float(rate)
    f0 = rng.uniform(100, 0.15 * rate)
    return np.round(5000 * np.sin(2 * np.pi * f0 * t * (1 + 0.3 * t)) + 1500 * rng.normal(size=n)).astype(np.int16)


def sweep_signals(geo):
    rng = np.random.default_rng(1500 + [g[0] for g in GEOMETRIES + [DEFAULT]].index(geo[0]))
    return [chirp_noise(rng, n, geo[1]) for n in SWEEP_LENGTHS]


def edge_lengths(flen, step):
    return [1, step - 1, step, step + 1, flen - 1, flen, flen + 1]


def edge_signals(geo):
    rng = np.random.default_rng(2000 + geo[6])
    return [rng.integers(-3000, 3001, size=n).astype(np.int16) for n in edge_lengths(geo[6], geo[7])]


def noise(rng, n):
    x = rng.integers(-5000, 5001, size=n).astype(np.int16)
    x[x == 0] = 1                                          # silence only where a test puts it
    return x


def silent_cases():
    """Digital silence beside audio at the default geometry (400 / 160): name -> list of int16 utterances.
    Pre-emphasis carries a loud sample one place into a zero stretch: x[n] - 0.97 x[n - 1]."""
    rng = np.random.default_rng(3000)
    a = np.zeros(2000, dtype=np.int16)
    a[:100] = noise(rng, 100)                              # frames 1 .. 12 silent; frame 1 is the B partner of loud frame 0
    b = noise(rng, 2000)
    b[:400] = 0                                            # frame 0: a silent A beside a loud B -- the only silent frame
    b2 = noise(rng, 2000)
    b2[159:560] = 0                                        # frame 1: a silent B beside a loud A -- the only silent frame
    c = noise(rng, 2500)
    c[700:1700] = 0                                        # frames 5 .. 8
    d = [noise(rng, 2000), np.zeros(800, dtype=np.int16), noise(rng, 1700)]    # 13 frames, 5 silent ones, 11
    return {"a": [a], "b": [b, b2], "c": [c], "d": d}


def quiet_loud_signals():
    """256 / 256 frames alternating between full-scale int16 noise and +-1 LSB noise, loud first and quiet first.  The last
    sample of every loud frame is 0, so that pre-emphasis carries nothing of it into the quiet frame behind."""
    rng = np.random.default_rng(4000)
    out = []
    for first_loud in (0, 1):
        x = np.zeros(3000, dtype=np.int16)
        for t in range(12):
            seg = x[256 * t:256 * (t + 1)]
            if t % 2 == first_loud:
                seg[:] = rng.integers(-32768, 32768, size=len(seg))
                seg[-1] = 0
            else:
                seg[:] = rng.integers(-1, 2, size=len(seg))
                seg[::7] = 1
        out.append(x)
    return out


POSITION_LENGTHS = (480, 4001, 800, 1920)                  # 3, 26, 5 and 12 frames at 400 / 160


def position_signals():
    rng = np.random.default_rng(5000)
    return [chirp_noise(rng, n, 16000) for n in POSITION_LENGTHS]


# ------------------------------------------------------------------ closed-form spectra (512 / 160: no padding)
def geometric_sum(psi, L, exact_one):
    """sum_{n < L} e^{i psi n}; exact_one: e^{i psi} is exactly 1 (decided in integers by the caller)."""
    if exact_one:
        return LD(L), LD(0)
    # (1 - z^L) / (1 - z), z = e^{i psi}
    nr, ni = 2 * np.sin(psi * L / 2) ** 2, -np.sin(psi * L)              # 1 - cos x = 2 sin^2 (x / 2), without the cancellation
    dr, di = 2 * np.sin(psi / 2) ** 2, -np.sin(psi)
    den = dr * dr + di * di
    return (nr * dr + ni * di) / den, (ni * dr - nr * di) / den


def closed_form_power(kind, a, n, s=None):
    """Power spectrum [T, 257] of the 512 / 160 frames of an n-sample signal WITHOUT a transform.
    kind "impulse": x[s] = a, 0 elsewhere -- after pre-emphasis two samples, a at s and -0.97 a at s + 1, so a frame that
    holds them at p, p + 1 has |a w[p] - 0.97 a w[p + 1] e^{-2 pi i k / 512}|^2 / 512;
    kind "constant": x = a; kind "alternating": x[n] = a[n % 2] -- after pre-emphasis c + d (-1)^n from sample 1 on, times
    the window 0.54 - 0.23 (e^{i th n} + e^{-i th n}), th = 2 pi / 511: six geometric series per bin."""
    flen, step = 512, 160
    T = frame_count(n, step)
    k = np.arange(NFFT // 2 + 1)
    w = hamming(flen)
    re = np.zeros((T, len(k)), dtype=LD)
    im = np.zeros((T, len(k)), dtype=LD)

    def add_sample(t, p, val):                             # one sample `val` at place p of frame t
        m = (p * k) % NFFT
        ang = 2 * PI * m.astype(LD) / NFFT
        re[t] += val * w[p] * np.cos(ang)
        im[t] -= val * w[p] * np.sin(ang)

    if kind == "impulse":
        for t in range(T):
            for g, val in ((s, LD(a)), (s + 1, -LD(0.97) * LD(a))):
                p = g - t * step
                if 0 <= p < flen and g < n:
                    add_sample(t, p, val)
        return (re * re + im * im) / NFFT
    x0, x1 = (LD(a), LD(a)) if kind == "constant" else (LD(a[0]), LD(a[1]))
    e_even, e_odd = x0 - LD(0.97) * x1, x1 - LD(0.97) * x0               # emphasized sample at an even / odd place >= 1
    c, d = (e_even + e_odd) / 2, (e_even - e_odd) / 2
    th = 2 * PI / (flen - 1)
    for t in range(T):
        L = min(flen, n - t * step)                        # the zero extension of `segment` cuts the series short
        sign = 1 if (t * step) % 2 == 0 else -1
        for alpha, j in ((LD(0.54), 0), (-LD(0.23), 1), (-LD(0.23), -1)):      # window terms e^{i j th n}
            for coef, half in ((c, 0), (d * sign, 1)):                         # signal terms e^{i pi half n}
                if coef == 0:
                    continue
                for kk in k:
                    # psi = j th + pi half - 2 pi kk / 512, the multiples of 2 pi / 512 reduced in integers
                    q = (256 * half - kk) % NFFT
                    psi = j * th + 2 * PI * LD(int(q)) / NFFT
                    gr, gi = geometric_sum(psi, L, exact_one=(j == 0 and q == 0))
                    re[t, kk] += alpha * coef * gr
                    im[t, kk] += alpha * coef * gi
        if t == 0:                                         # sample 0 is taken as it is
            re[0] += (x0 - (c + d)) * w[0]
    return (re * re + im * im) / NFFT


def closed_form_cases():
    """name -> (signal int16, power spectrum [T, 257]) on the 512 / 160 geometry."""
    n = 2000
    out = {}
    for name, s in (("impulse at 700", 700), ("impulse at 860", 860)):     # one step apart: the frames that hold it swap slots
        x = np.zeros(n, dtype=np.int16)
        x[s] = 12345
        out[name] = (x, closed_form_power("impulse", 12345, n, s))
    x = np.empty(n, dtype=np.int16)
    x[0::2], x[1::2] = 32767, -32768                       # all the energy at bin 256
    out["alternating"] = (x, closed_form_power("alternating", (32767, -32768), n))
    out["constant"] = (np.full(n, 20000, dtype=np.int16), closed_form_power("constant", 20000, n))
    return out
