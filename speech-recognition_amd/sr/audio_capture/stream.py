# -*- coding: utf-8 -*-
"""Endpoint detection for audio that is still arriving.  The reference's `record_callback` (record.py:116-174) is a
streaming algorithm: it runs once per audio chunk and carries `level`, `background`, the two counters and
`started_speech` between calls.  `StreamingEndpointer` is that carried form on the GPU (csrc/gh_endpoint_stream.hip) for
many streams at once, and `gate` turns its events into the pieces of audio an `OnlineDecoder` should take."""
import numpy as np

from ..recognition import _hip
from .record import _derived

__all__ = ["StreamingEndpointer"]


def _stream_config(config, sample_rate):
    cfg = _derived(config, sample_rate)
    width, stride = int(cfg['samples per frame']), int(cfg['frame stride'])
    if width % stride:
        raise ValueError("frames of %d samples every %d: a stream needs 'samples per frame' to be a multiple of 'frame stride' -- "
                         "otherwise the reference's frames fall behind the audio by %d samples per chunk, without bound; such "
                         "recordings are for detect_endpoints" % (width, stride, width - int(width / stride) * stride))
    return cfg


class StreamingEndpointer:
    """`detect_endpoints` for `n_streams` recordings that are still arriving: every `push` hands each stream a chunk of
    int16 PCM and returns the start / end events its newly complete frames produced.

        ep = StreamingEndpointer(n_streams=64, config=default_config(16000))
        r = ep.push([3, 7], [pcm_of_3, pcm_of_7])               # 1-D int16 arrays of any length, 0 included
        r = ep.push([3], [last_piece], end=[True])                # the recording ends: an open segment is closed
        ep.reset([3])                                             # id 3 is free for a new recording

    However a recording is cut, its stream's events and per-frame values are exactly those of `detect_endpoints(...,
    max_segments=large)` on the whole recording: the detector re-arms after every end with all state left as it is, with
    no cap and no stop.  `push` returns a dict:
      stream, kind, sample, open   one entry per event, ordered by position in `ids`, then by time; kind 0 = start (the
                                   reference's speech_start_index), 1 = end (speech_end_index); a recording that ends while
                                   speech is open gets an end event at its last sample with open = True
      frames_done, started         per id, after the push
    and with want_frames the ragged `is_speech`, `level`, `background`, `energy` of the newly classified frames and their
    `frame_off`.  config: as for `detect_endpoints` (None: the default config at 8 kHz); 'samples per frame' must be a
    multiple of 'frame stride' (ValueError otherwise: the 16 kHz 400 / 160 framing is for `detect_endpoints`).  Bad
    arguments -- an id twice or out of range, a chunk that is not 1-D int16 or longer than `max_chunk` samples, audio for
    a stream that has ended -- raise ValueError before the GPU is touched, and no stream moves.

    `gate` is host logic on top of `push` for an `OnlineDecoder` (`dec.online(..., frontend=fe, endpointer=ep)`)."""

    def __init__(self, n_streams, config=None, max_chunk=16000, device=None):
        if int(n_streams) < 1 or int(max_chunk) < 1:
            raise ValueError("n_streams and max_chunk must be positive")
        self.config = _stream_config(config, 8000)
        self.n_streams, self.max_chunk = int(n_streams), int(max_chunk)
        self.width, self.stride = int(self.config['samples per frame']), int(self.config['frame stride'])
        self.boundary = int(self.config['start boundary'])
        self.sample_rate = int(self.config['sample rate'])
        self.carry_cap = 2 * self.width - self.stride                 # the carry is always shorter than this
        self.ctx = _hip.default_context(device)
        self.backend = _hip.EndpointStream(self.ctx, self.n_streams, self.config, self.max_chunk)
        self._samples = np.zeros(self.n_streams, dtype=np.int64)      # what the backend holds, for the checks below
        self._ended = np.zeros(self.n_streams, dtype=bool)
        # the gate: per stream the samples [_base, _samples) and the utterance that is open (None: closed)
        self._keep = [np.zeros(0, dtype=np.int16) for _ in range(self.n_streams)]
        self._base = np.zeros(self.n_streams, dtype=np.int64)
        self._utt = [None] * self.n_streams                           # dict(begin, sent, stop): stop set = end sample not yet arrived

    # ------------------------------------------------------------------ counts
    def frames_after(self, n_samples):
        """Frames a stream has classified after `n_samples` samples (a scalar or an array): the reference's count from
        whole chunks of 'samples per frame' samples."""
        n = np.asarray(n_samples, dtype=np.int64)
        c = n // self.width
        out = np.where(c == 0, 0, 1 + (self.width // self.stride) * (c - 1))
        return out if out.ndim else int(out)

    def carry_after(self, n_samples):
        """Samples a stream carries after `n_samples` samples: from the first sample of the next frame to classify."""
        n = np.asarray(n_samples, dtype=np.int64)
        out = n - self.frames_after(n) * self.stride
        return out if out.ndim else int(out)

    @property
    def max_piece(self):
        """The largest piece `gate` can hand out: an utterance opens at most 'start boundary' samples before the first
        carried sample and takes everything up to the newest one."""
        return self.boundary + self.carry_cap + self.max_chunk

    @property
    def min_utterance(self):
        """The shortest utterance `gate` can hand out: a recording that ends at the frame at which speech started."""
        first = (max(int(self.config['speech threshold']), 0) + 1) * self.stride
        return self.width + min(self.boundary, first)

    @property
    def samples(self):
        """Samples every stream has taken since its last reset: int64 [n_streams]."""
        return self._samples.copy()

    # ------------------------------------------------------------------ push
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
        """Every check of `push` without the push: (ids, chunks, end).  Moves nothing."""
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
            raise ValueError("stream %d has ended: reset it before it takes a new recording" % ids[np.flatnonzero(self._ended[ids])[0]])
        return ids, chunks, end

    def push(self, ids, chunks, end=None, want_frames=False):
        """Stream ids[i] takes the samples chunks[i] (1-D int16, 0 .. max_chunk of them); end[i] true ends its recording."""
        return self._push(*self.plan(ids, chunks, end), want_frames=want_frames)

    def _push(self, ids, chunks, end, want_frames=False):
        off = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum([len(c) for c in chunks], out=off[1:])
        pcm = np.concatenate(chunks) if len(chunks) else np.zeros(0, dtype=np.int16)
        r = self.backend.push(ids, pcm, off, end.astype(np.uint8), want_frames=want_frames)
        self._samples[ids] = self._samples[ids] + np.diff(off)
        self._ended[ids] |= end
        assert np.array_equal(r["frames_done"], self.frames_after(self._samples[ids]))
        return r

    def reset(self, ids=None):
        """The streams `ids` (None: all) start a new recording at sample 0; the gate forgets what it kept of them."""
        ids = None if ids is None else self._ids(ids, distinct=False)
        self.backend.reset(ids)
        if ids is None:
            self._samples[:] = 0
            self._ended[:] = False
        else:
            self._samples[ids] = 0
            self._ended[ids] = False
        for k in (range(self.n_streams) if ids is None else ids):
            self._keep[int(k)], self._base[int(k)], self._utt[int(k)] = np.zeros(0, dtype=np.int16), 0, None

    def close(self):
        self.backend.close()

    # ------------------------------------------------------------------ the gate
    def gate(self, ids, chunks, end=None):
        """`push`, and what an `OnlineDecoder` should take of the audio: a list of rounds `(ids, pieces, end_flags, ranges)`
        that can go straight into `push_audio` one after the other (ids are distinct within a round; a stream with several
        events in this push has a piece in several rounds).  ranges[i] is None while the utterance goes on and `(begin,
        stop, open)` in recording sample coordinates for the piece that ends it (end_flags[i] true).

          closed               audio is not forwarded
          start at s           the utterance opens at begin = max(s - 'start boundary', 0) and takes everything from there
          open                 the audio is forwarded up to the end of the next frame to classify (+ 1 sample): the
                               classifier is behind the audio by the carry, and an end it finds later must not lie before
                               what has been handed out; the rest (fewer than width - stride samples) waits for the next push
          end at e             the utterance takes the samples up to and including e: stop = e + 1
          e not yet arrived    (the end frame is the last frame of the last chunk) the utterance takes the first sample of
                               the next push; at the end of the recording it is clipped to n instead
          recording ends open  the utterance closes with stop = n, open = True

        These are the slices of `trim_ranges` on the offline detection -- except that a recording without a segment yields
        no utterance, where `trim_ranges` keeps it whole.  The gate keeps, per stream, the samples back to 'start
        boundary' before the carry: a start event of a push lies at or behind the first carried sample."""
        ids, chunks, end = self.plan(ids, chunks, end)
        n0 = self._samples[ids].copy()
        carried = np.asarray(self.frames_after(n0)).reshape(-1) * self.stride        # first carried sample before the push
        r = self._push(ids, chunks, end)
        events = [[] for _ in ids]
        pos = {int(k): u for u, k in enumerate(ids)}
        for k, kind, sample, is_open in zip(r["stream"], r["kind"], r["sample"], r["open"]):
            events[pos[int(k)]].append((int(kind), int(sample), bool(is_open)))
        per_stream = []
        for u, k in enumerate(ids):
            k = int(k)
            buf = np.concatenate([self._keep[k], chunks[u]])
            base, n1, fin = int(self._base[k]), int(n0[u]) + len(chunks[u]), bool(end[u])
            cut = lambda a, b: buf[a - base:b - base]
            pieces, utt = [], self._utt[k]
            if utt is not None and utt["stop"] is not None:          # an end whose last sample had not arrived
                stop = min(utt["stop"], n1)
                if stop == utt["stop"] or fin:
                    pieces.append((cut(utt["sent"], stop), True, (utt["begin"], stop, False)))
                    utt = None
            for kind, sample, is_open in events[u]:
                if kind == 0:
                    assert utt is None and sample >= carried[u]
                    begin = max(sample - self.boundary, 0)
                    assert begin >= base
                    utt = dict(begin=begin, sent=begin, stop=None)
                    continue
                assert utt is not None and utt["stop"] is None
                stop = n1 if is_open else sample + 1
                if stop <= n1 or fin:
                    stop = min(stop, n1)
                    pieces.append((cut(utt["sent"], stop), True, (utt["begin"], stop, is_open)))
                    utt = None
                else:
                    utt["stop"] = stop
            if utt is not None:
                # the classifier is behind the audio by the carry: an end found later lies at or behind the end of the next
                # frame to classify, so that far -- and no farther -- the audio of an open utterance can go on now
                limit = n1 if utt["stop"] is not None else min(n1, int(self.frames_after(n1)) * self.stride + self.width + 1)
                if utt["sent"] < limit:
                    pieces.append((cut(utt["sent"], limit), False, None))
                    utt["sent"] = limit
            self._utt[k] = None if fin else utt
            per_stream.append(pieces)
            # keep what a later start can reach back to
            nb = max(int(self.frames_after(n1)) * self.stride - self.boundary, 0)
            self._keep[k], self._base[k] = (buf[nb - base:].copy(), nb) if nb > base else (buf, base)
        rounds = []
        for j in range(max([len(p) for p in per_stream] + [0])):
            who = [u for u, p in enumerate(per_stream) if len(p) > j]
            rounds.append((ids[who], [per_stream[u][j][0] for u in who], np.array([per_stream[u][j][1] for u in who], dtype=bool),
                           [per_stream[u][j][2] for u in who]))
        return rounds
