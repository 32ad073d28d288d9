# -*- coding: utf-8 -*-
"""`sr.feature` -- the reference's feature extraction in front of the recognition hot path
(sr/feature/feature.py), on the GPU: `mfcc_features` (:43-82) and `standardize` (:85-88).
`mfcc_features` keeps the reference's signature (a wav path in, `(filter_banks, mfcc)` out);
`mfcc_from_signals` is the batched entry point on in-memory audio, and
`features_from_signals` chains MFCC -> delta -> delta-delta -> standardize on the device into a resident
batch (what `load_wav_as_mfcc`, sr/core.py:25-44, returns -- for many utterances, without a host round trip).
`StreamingFrontend` is the same front-end for audio that is still arriving: int16 chunks in, the frames that became final
out, with a FIXED normalisation `(mean, std)` in place of the per-utterance one (`feature_stats` computes a pair,
`features_from_signals(..., normalize=)` applies it to whole utterances) or a `RunningNorm`: the causal running mean /
variance normalisation that starts at such a pair and moves to the stream's own statistics."""
import numpy as np

from ..recognition import _hip

__all__ = ["standardize", "mfcc_features", "mfcc_from_signals", "features_from_signals", "feature_stats", "frames_ready",
           "StreamingFrontend", "RunningNorm"]


def standardize(data):
    """(data - mean) / std per column, population std.  Like the reference the mean is
    subtracted from the caller's array IN PLACE (`data -= mean`) and a new array is returned."""
    data -= np.mean(data, axis=0)
    ctx = _hip.default_context()
    b = _hip.Batch(ctx, cepstra=[data], frontend_mode=2)
    try:
        return b.features()[0].copy()
    finally:
        b.close()


def mfcc_from_signals(signals, sample_rate=16000, frame_size=0.025, frame_stride=0.01, low_freq=80, high_freq=None,
                      device=None):
    """mfcc_features for a list of 1-D sample arrays (int16 as read from a wav file, or float):
    returns ([T_u,40] log10 mel filterbank energies, [T_u,13] cepstra), one launch for all of them."""
    return _hip.mfcc(_hip.default_context(device), signals, sample_rate, (frame_size, frame_stride, low_freq, high_freq))


def mfcc_features(path_file, frame_size=0.025, frame_stride=0.01, low_freq=80, high_freq=None):
    """feature.py:43-82: wav file -> (filter_banks [T,40], mfcc [T,13])."""
    from scipy.io import wavfile
    sample_rate, signal = wavfile.read(path_file)
    fb, mf = mfcc_from_signals([signal], sample_rate, frame_size, frame_stride, low_freq, high_freq)
    return fb[0], mf[0]


def _mfcc_params(mfcc_kw):
    unknown = set(mfcc_kw) - {"frame_size", "frame_stride", "low_freq", "high_freq"}
    if unknown:
        raise TypeError("unknown MFCC parameter(s): %s" % ", ".join(sorted(unknown)))
    return (mfcc_kw.get("frame_size", 0.025), mfcc_kw.get("frame_stride", 0.01), mfcc_kw.get("low_freq", 80), mfcc_kw.get("high_freq"))


def _normalize_pair(normalize):
    mean, std = (np.asarray(a, dtype=np.float64).reshape(-1) for a in normalize)
    if len(mean) != 39 or len(std) != 39 or not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std != 0)):
        raise ValueError("normalize = (mean [39], std [39]), finite, std nonzero")
    return mean, std


class RunningNorm:
    """The causal running mean / variance normalisation as a `normalize=` value: the statistics start at
    `prior` = (mean [39], std [39]) (e.g. `feature_stats` of training audio), which counts as `prior_frames` frames, and
    move to the stream's own as frames arrive; the deviation never falls below `min_std` times the prior's.  Per frame,
    in fp64 on the raw value rounded to the batch dtype: d = r - mean, S += d, Q += d d, n = prior_frames + c, a = S / n,
    v = (prior_frames std^2 + Q) / n - a^2, y = (d - a) / sqrt(max(v, (min_std std)^2)).  prior_frames -> infinity gives
    the fixed map (r - mean) / std; with prior_frames = 0 the last frame of an utterance is the last row of `standardize`.
    per = "utterance": a `StreamingFrontend`'s `reset` clears a stream's statistics, every utterance is normalised alone
    (what `features_from_signals` computes for training); per = "stream": they survive `reset` -- successive utterances of
    one microphone keep adapting -- until `reset_stats` (an online decoder's `reset` calls it: a new recording)."""

    def __init__(self, prior, prior_frames=100, min_std=0.1, per="utterance"):
        try:
            mean, std = (np.asarray(a, dtype=np.float64).reshape(-1) for a in prior)
        except (TypeError, ValueError):
            raise ValueError("prior = (mean [39], std [39])")
        if len(mean) != 39 or len(std) != 39 or not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std > 0)):
            raise ValueError("prior = (mean [39], std [39]), finite, std > 0")
        try:
            pf, ms = float(prior_frames), float(min_std)
        except (TypeError, ValueError):
            raise ValueError("prior_frames and min_std are numbers")
        if not (np.isfinite(pf) and pf >= 0 and pf == np.floor(pf) and pf <= 2.0 ** 52):
            raise ValueError("prior_frames = %r: a whole number >= 0" % (prior_frames,))
        if not (np.isfinite(ms) and 0 < ms <= 1):
            raise ValueError("min_std = %r: 0 < min_std <= 1" % (min_std,))
        if per not in ("utterance", "stream"):
            raise ValueError("per = %r: 'utterance' or 'stream'" % (per,))
        self.prior, self.prior_frames, self.min_std, self.per = (mean, std), pf, ms, per


def features_from_signals(signals, sample_rate=16000, dtype=np.float64, device=None, endpoints=None, max_segments=1, normalize=None,
                          **mfcc_kw):
    """Audio in, resident 39-dimensional batch out: MFCC -> [ceps | delta | delta-delta] -> standardize,
    all on the device; returns the `_hip.Batch` ready for `loglik` / decoding.

    normalize=(mean [39], std [39]): the FIXED map (x - mean) / std of `StreamingFrontend` in place of the per-utterance
    `standardize` -- the raw stacked features (rounded to `dtype`) go through `Batch.affine`: bitwise what a stream with the
    same pair emits for the utterance, wherever it stands in the batch (frames share an FFT in pairs, and pair inside their
    utterance).  `feature_stats` computes such a pair from training audio.
    normalize=RunningNorm(...): the causal running normalisation instead, through `Batch.running_norm` on the same raw
    batch, every utterance alone from zero statistics (`per` plays no part here) -- the features to train the models of
    a `StreamingFrontend(normalize=RunningNorm(...))` with, and bitwise what such a stream emits for the utterance.

    endpoints: an AudioRecorder config (sr.audio_capture; True: the reference's default config at `sample_rate`) -- the
    1-D int16 recordings are first cut down to their speech on the device (`detect_endpoints`, up to `max_segments`
    segments each, every one trimmed like `get_samples`; a recording without a segment stays whole) and the batch holds
    one utterance per segment in recording order.  `batch.endpoints` is the result of `detect_endpoints` plus
    `recording` [batch.U], the recording of every utterance.  The samples are uploaded once and do not come back; only
    the per-recording indices do.  A dict whose 'sample rate' differs from `sample_rate` is a ValueError."""
    prm = (mfcc_kw.get("frame_size", 0.025), mfcc_kw.get("frame_stride", 0.01), mfcc_kw.get("low_freq", 80),
           mfcc_kw.get("high_freq"))
    mode = {}
    finish = lambda b: b
    if isinstance(normalize, RunningNorm):
        run = normalize
        finish = lambda b: b.running_norm(run.prior[0], run.prior[1], run.prior_frames, run.min_std)
        mode = dict(frontend_mode=1)
    elif normalize is not None:
        pair = _normalize_pair(normalize)
        finish = lambda b: b.affine(*pair)
        mode = dict(frontend_mode=1)
    if endpoints is None or endpoints is False:
        b = _hip.Batch(_hip.default_context(device), pcm=signals, sample_rate=sample_rate, mfcc_params=prm, dtype=dtype, **mode)
        return finish(b)
    from ..audio_capture.record import _check_signals, _derived      # (`sr.audio_capture.record` the name is the function)
    cfg = _derived(None if endpoints is True else endpoints, sample_rate)
    if cfg['sample rate'] != sample_rate:
        raise ValueError("the endpoint config is for %r Hz, the signals are at %r Hz" % (cfg['sample rate'], sample_rate))
    if int(max_segments) < 1:
        raise ValueError("max_segments = %r" % (max_segments,))
    sigs = _check_signals(signals)
    b = _hip.Batch(_hip.default_context(device), pcm=sigs, sample_rate=sample_rate, mfcc_params=prm, dtype=dtype,
                   endpoints=cfg, max_segments=int(max_segments), **mode)
    return finish(b)


def feature_stats(signals, sample_rate=16000, device=None, **mfcc_kw):
    """(mean [39], std [39]) over ALL frames of `signals` of the raw [ceps | delta | delta-delta] features (fp64, population
    std, computed on the host): a `normalize=` pair for `StreamingFrontend` and `features_from_signals`."""
    b = _hip.Batch(_hip.default_context(device), pcm=signals, sample_rate=sample_rate, mfcc_params=_mfcc_params(mfcc_kw), frontend_mode=1)
    try:
        x = np.concatenate(b.features())
    finally:
        b.close()
    return x.mean(axis=0), x.std(axis=0)


def frames_ready(n_samples, ended=False, sample_rate=16000, **mfcc_kw):
    """Feature frames a stream has emitted after `n_samples` samples (a scalar or an array): see `_hip.stream_frames_ready`."""
    fs, st = _mfcc_params(mfcc_kw)[:2]
    return _hip.stream_frames_ready(n_samples, int(float(fs) * int(sample_rate)), int(float(st) * int(sample_rate)), ended)


class StreamingFrontend:
    """The device front-end for audio that is still arriving: `n_streams` utterances take int16 PCM chunk by chunk and every
    `push` returns, as a resident `_hip.Batch`, exactly the 39-dimensional frames that have become final.

        fe = StreamingFrontend(n_streams=64, normalize=feature_stats(training_signals))
        batch = fe.push([3, 7], [pcm_of_3, pcm_of_7])           # 1-D int16 arrays of any length, 0 included
        batch = fe.push([3], [last_piece], end=[True])            # ends the utterance: all its remaining frames
        fe.reset([3])                                             # id 3 is free for a new utterance

    A stream's concatenated frames are bitwise `features_from_signals([signal], normalize=...)` of its utterance alone,
    however it was cut.  While a stream is open it has emitted `frames_ready(n)` frames after n samples (a frame is final
    when the cepstra of the two frames behind it exist, and those are computed in pairs); the end flushes the rest.
    `normalize` is a FIXED `(mean [39], std [39])`, None for raw features, or a `RunningNorm`: per-utterance `standardize`
    needs the whole utterance, the running normalisation is its causal stand-in (the front-end then has `reset_stats` and
    `norm_frames`, and `features_from_signals(..., normalize=` the same `RunningNorm)` gives the matching training
    features).  Bad arguments -- an id twice or out of range, a chunk that is not 1-D int16 or longer than `max_chunk`
    samples, audio for a stream that has ended, an end with fewer than 2 frames -- raise ValueError before the GPU is
    touched, and no stream moves."""

    def __init__(self, n_streams, sample_rate=16000, normalize=None, max_chunk=16000, dtype=np.float64, device=None, **mfcc_kw):
        if int(n_streams) < 1 or int(max_chunk) < 1:
            raise ValueError("n_streams and max_chunk must be positive")
        self.n_streams, self.sample_rate, self.max_chunk = int(n_streams), int(sample_rate), int(max_chunk)
        self.dtype = np.dtype(dtype)
        self.running = normalize if isinstance(normalize, RunningNorm) else None
        self.normalize = None if normalize is None or self.running else _normalize_pair(normalize)
        self.mfcc_params = _mfcc_params(mfcc_kw)
        self.flen = int(float(self.mfcc_params[0]) * self.sample_rate)
        self.step = int(float(self.mfcc_params[1]) * self.sample_rate)
        self.D = 39
        self.ctx = _hip.default_context(device)
        if self.running is None:
            self.backend = _hip.StreamFrontend(self.ctx, self.n_streams, self.sample_rate, self.mfcc_params, self.max_chunk, self.dtype,
                                               self.normalize)
        else:
            self.backend = _hip.RunningStreamFrontend(self.ctx, self.n_streams, self.sample_rate, self.mfcc_params, self.max_chunk,
                                                      self.dtype, self.running.prior, self.running.prior_frames, self.running.min_std,
                                                      self.running.per == "stream")
            self._norm_frames = np.zeros(self.n_streams, dtype=np.int64)  # what the backend's statistics hold
        self._samples = np.zeros(self.n_streams, dtype=np.int64)      # what the backend holds, for the checks below
        self._ended = np.zeros(self.n_streams, dtype=bool)

    def frames_ready(self, n_samples, ended=False):
        """Frames a stream of this front-end has emitted after `n_samples` samples (a scalar or an array)."""
        return _hip.stream_frames_ready(n_samples, self.flen, self.step, ended)

    @property
    def samples(self):
        """Samples every stream has taken since its last reset: int64 [n_streams]."""
        return self._samples.copy()

    def _ids(self, ids, distinct=True):
        a = np.asarray(ids)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("ids must be a one-dimensional sequence of stream indices")
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.n_streams):
            raise ValueError("stream ids must lie in [0, %d)" % self.n_streams)
        if distinct and len(np.unique(a)) != len(a):
            raise ValueError("a stream is named twice in one push")
        return a

    def plan(self, ids, chunks, end=None):
        """Every check of `push` without the push: (ids, chunks, end, frames each stream would emit).  Moves nothing."""
        ids = self._ids(ids)
        if len(chunks) != len(ids):
            raise ValueError("%d chunks for %d ids" % (len(chunks), len(ids)))
        chunks = [np.asarray(c) for c in chunks]
        for c in chunks:
            if c.ndim != 1 or c.dtype != np.int16:
                raise ValueError("a chunk must be a one-dimensional int16 array, not %s of shape %r" % (c.dtype, c.shape))
            if len(c) > self.max_chunk:
                raise ValueError("a chunk of %d samples, max_chunk %d" % (len(c), self.max_chunk))
        end = np.zeros(len(ids), dtype=bool) if end is None else np.asarray(end, dtype=bool).reshape(-1)
        if len(end) != len(ids):
            raise ValueError("%d end flags for %d ids" % (len(end), len(ids)))
        if np.any(self._ended[ids]):
            raise ValueError("stream %d has ended: reset it before it takes a new utterance" % ids[np.flatnonzero(self._ended[ids])[0]])
        after = self._samples[ids] + np.array([len(c) for c in chunks], dtype=np.int64)
        short = end & (-(-after // self.step) < 2)
        if np.any(short):
            k = int(np.flatnonzero(short)[0])
            raise ValueError("stream %d would end with %d samples: fewer than 2 frames" % (ids[k], after[k]))
        counts = self.frames_ready(after, end) - self.frames_ready(self._samples[ids])
        return ids, chunks, end, np.asarray(counts, dtype=np.int64).reshape(-1)

    def push(self, ids, chunks, end=None):
        """Stream ids[i] takes the samples chunks[i] (1-D int16, 0 .. max_chunk of them); end[i] true ends its utterance.
        Returns the `_hip.Batch` of the frames that became final: len(ids) utterances in the order of `ids`, ragged."""
        return self._push(*self.plan(ids, chunks, end))

    def _push(self, ids, chunks, end, counts):
        off = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum([len(c) for c in chunks], out=off[1:])
        pcm = np.concatenate(chunks) if len(chunks) else np.zeros(0, dtype=np.int16)
        batch = self.backend.push(ids, pcm, off, end.astype(np.uint8))
        assert np.array_equal(batch.lengths, counts)
        self._samples[ids] = self._samples[ids] + np.diff(off)
        self._ended[ids] |= end
        if self.running is not None:
            self._norm_frames[ids] = self._norm_frames[ids] + counts
        return batch

    def reset(self, ids=None):
        """The streams `ids` (None: all) start a new utterance at sample 0."""
        ids = None if ids is None else self._ids(ids, distinct=False)
        self.backend.reset(ids)
        if ids is None:
            self._samples[:] = 0
            self._ended[:] = False
        else:
            self._samples[ids] = 0
            self._ended[ids] = False
        if self.running is not None and self.running.per == "utterance":
            self._norm_frames[slice(None) if ids is None else ids] = 0

    @property
    def norm_frames(self):
        """Frames the running statistics of every stream hold: int64 [n_streams] (zeros without a `RunningNorm`)."""
        return self._norm_frames.copy() if self.running is not None else np.zeros(self.n_streams, dtype=np.int64)

    def reset_stats(self, ids=None):
        """The running statistics of streams `ids` (None: all) start again at the prior -- a new speaker or microphone on the
        stream.  With per="utterance" `reset` has done that already; without a `RunningNorm` there is nothing to clear."""
        ids = None if ids is None else self._ids(ids, distinct=False)
        if self.running is None:
            return
        self.backend.reset_stats(ids)
        self._norm_frames[slice(None) if ids is None else ids] = 0

    def close(self):
        self.backend.close()
