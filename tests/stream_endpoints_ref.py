# -*- coding: utf-8 -*-
"""Host restatement of the streaming endpoint detector for the tests (numpy only, no GPU):

* `initial_state` / `carried_step`: the carried detector -- state in, chunk in, state and events out.  It is
  `audio_capture_ref.detect` cut open between two frames: the same numpy operations on the same values in the same order, so
  that whatever way a recording is fed, events AND per-frame arrays equal `detect(whole, cfg, max_segments=large)` exactly;
* `feed`: a whole recording through `carried_step` with given chunk lengths;
* `carry_brute` / `frames_brute`: the frame count and the carry spelled out chunk by chunk, as the reference's callback would
  see them;
* `FakeEndpointStream`: a double of `_hip.EndpointStream` on `carried_step`, for the host logic of `StreamingEndpointer`,
  its gate and `OnlineDecoder.push_recording`."""
import numpy as np

import audio_capture_ref as A


def initial_state():
    return dict(n=0, frames=0, carry=np.zeros(0, dtype=np.int16), level=np.float64(0), bg=0, attr=False, started=False,
                speech=0, silence=0)


def frames_brute(n, width, stride):
    """The callback's frames after n samples: it is called with whole chunks of `width` samples; the first makes frame 0,
    every later one appends int(width / stride) frames (record.py:132-147)."""
    frames, chunks = 0, 0
    while (chunks + 1) * width <= n:
        chunks += 1
        frames += 1 if chunks == 1 else int(width / stride)
    return frames


def carry_brute(n, width, stride):
    """Samples from the first sample of the next frame to classify (frame 0 counts as classified) up to the last one."""
    return n - frames_brute(n, width, stride) * stride


def carried_step(state, chunk, cfg, end=False):
    """(new state, events [(kind, sample, open)], dict of the new frames' is_speech / level / background / energy)."""
    width, stride = cfg['samples per frame'], cfg['frame stride']
    ff, adj = cfg['forget factor'], cfg['adjustment']
    onset, offset = cfg['onset threshold'], cfg['offset threshold']
    st = dict(state)
    chunk = np.asarray(chunk, dtype=np.int16)
    cbase = st["frames"] * stride                          # absolute index of carry[0]
    buf = np.concatenate([st["carry"], chunk])
    assert len(st["carry"]) == st["n"] - cbase
    n = st["n"] + len(chunk)
    f_first, f_end = st["frames"], A.frame_count(n, width, stride)
    nf = f_end - f_first
    # energies of the new frames: exact integer sums, then the expression of audio_capture_ref.energies
    sq = buf.astype(np.int64) ** 2
    s = np.array([sq[i * stride - cbase:i * stride - cbase + width].sum() for i in range(f_first, f_end)], dtype=np.int64)
    E = np.where(s <= 1, 0.0, 10 * np.log10(np.maximum(s, 2))) if nf else np.zeros(0)
    if nf and f_first == 0:
        E[0] = 0.0
    attr, level, background, energy = np.zeros(nf, dtype=bool), np.zeros(nf), np.zeros(nf), np.zeros(nf)
    events = []
    lv, bg, prev_attr, started, speech, silence = st["level"], st["bg"], st["attr"], st["started"], st["speech"], st["silence"]
    if f_first == 0 and nf:
        bg += E[0]                                        # detect sums E[0..10] at frame 10, E[0] = 0 first
    for i in range(max(f_first, 1), f_end):
        k = i - f_first
        e = E[k]
        energy[k] = e
        is_speech = False
        now = False
        if i <= 10:
            lv = e
        else:
            lv = (lv + (ff * e)) / (ff + 1)
            is_speech = bool(prev_attr)
        if i <= 10:
            bg += e
        if i >= 10:
            if i == 10:
                bg /= 10
            else:
                bg += (e - bg) * adj
            if lv < bg:
                lv = bg
            elif lv - bg > onset:
                now = True
                is_speech = True
            elif lv - bg < offset:
                now = False
                is_speech = False
            else:
                now = is_speech
            attr[k] = now
            background[k] = bg
        level[k] = lv
        prev_attr = now
        if is_speech:
            speech += 1
            silence = 0
        else:
            silence += 1
            speech = 0
        if speech > cfg['speech threshold'] and not started:
            silence = 0
            started = True
            events.append((0, i * stride, False))
        elif silence > cfg['silence threshold'] and started:
            started = False
            events.append((1, i * stride + width, False))
    if end and started:
        events.append((1, n - 1, True))
    cnew = f_end * stride
    st.update(n=n, frames=f_end, carry=buf[cnew - cbase:].copy(), level=np.float64(lv), bg=bg, attr=prev_attr, started=started,
              speech=speech, silence=silence)
    return st, events, dict(is_speech=attr, level=level, background=background, energy=energy)


def feed(signal, cfg, lengths, end=True):
    """The recording through `carried_step` in chunks of `lengths` (they sum to len(signal)); the end flag rides on the
    last chunk.  Returns (events, per-frame dict concatenated, final state, longest carry seen)."""
    assert sum(lengths) == len(signal)
    st, events, parts, pos, longest = initial_state(), [], [], 0, 0
    for j, c in enumerate(lengths):
        st, ev, fr = carried_step(st, signal[pos:pos + c], cfg, end=end and j == len(lengths) - 1)
        pos += c
        events += ev
        parts.append(fr)
        longest = max(longest, len(st["carry"]))
    if not lengths:
        st, ev, fr = carried_step(st, signal[:0], cfg, end=end)
        events, parts = ev, [fr]
    frames = {k: np.concatenate([p[k] for p in parts]) for k in ("is_speech", "level", "background", "energy")}
    return events, frames, st, longest


def segments_of(events):
    """(starts, ends, open) as `audio_capture_ref.detect` returns them, from an event list."""
    starts = [s for k, s, _ in events if k == 0]
    ends = [s for k, s, _ in events if k == 1]
    return starts, ends, any(o for _, _, o in events)


class FakeEndpointStream:
    """`_hip.EndpointStream` on the host.  Like the real one it trusts its caller's checks and asserts them."""
    pushes = 0

    def __init__(self, ctx, n_streams, cfg, max_chunk=16000):
        self.ctx, self.n_streams, self.cfg, self.max_chunk = ctx, int(n_streams), dict(cfg), int(max_chunk)
        assert cfg['samples per frame'] % cfg['frame stride'] == 0
        self.reset()

    def reset(self, ids=None):
        if ids is None:
            self.state = [initial_state() for _ in range(self.n_streams)]
            self.over = [False] * self.n_streams
            return
        for k in ids:
            self.state[int(k)], self.over[int(k)] = initial_state(), False

    def samples(self):
        return np.array([s["n"] for s in self.state], dtype=np.int64)

    def push(self, ids, samples, sample_off, end=None, want_frames=False):
        type(self).pushes += 1
        ids = np.asarray(ids, dtype=np.int64)
        assert samples.dtype == np.int16 and len(sample_off) == len(ids) + 1 and len(set(ids.tolist())) == len(ids)
        assert len(ids) == 0 or (ids.min() >= 0 and ids.max() < self.n_streams)
        ev, done, started, frames = [], [], [], []
        for u, k in enumerate(ids):
            chunk = samples[sample_off[u]:sample_off[u + 1]]
            fin = bool(end is not None and end[u])
            assert len(chunk) <= self.max_chunk and not self.over[k]
            self.state[k], e, fr = carried_step(self.state[k], chunk, self.cfg, end=fin)
            assert len(self.state[k]["carry"]) < 2 * self.cfg['samples per frame'] - self.cfg['frame stride']
            self.over[k] = fin
            ev += [(int(k),) + x for x in e]
            done.append(self.state[k]["frames"])
            started.append(self.state[k]["started"])
            frames.append(fr)
        r = dict(stream=np.array([x[0] for x in ev], dtype=np.int64), kind=np.array([x[1] for x in ev], dtype=np.int64),
                 sample=np.array([x[2] for x in ev], dtype=np.int64), open=np.array([x[3] for x in ev], dtype=bool),
                 frames_done=np.array(done, dtype=np.int64), started=np.array(started, dtype=bool))
        if want_frames:
            r["frame_off"] = np.concatenate([[0], np.cumsum([len(f["level"]) for f in frames])]).astype(np.int64)
            for key in ("is_speech", "level", "background", "energy"):
                r[key] = [f[key] for f in frames]
        return r

    def close(self):
        pass


# ------------------------------------------------------------------ the recordings and cuttings both test files use
CONFIGS = [
    ("default 8 kHz", dict(A.DEFAULT_CONFIG)),
    ("8 kHz, 240 / 80 samples, forget factor 5",
     dict(A.DEFAULT_CONFIG, **{'forget factor': 5, 'frame time': 0.03, 'adjustment': 0.05, 'onset threshold': 2.5,
                               'offset threshold': 1.0, 'silence threshold': 200, 'speech threshold': 60})),
    ("11025 Hz, 220 / 110 samples (Q = 2)",
     dict(A.DEFAULT_CONFIG, **{'sample rate': 11025, 'forget factor': 2, 'silence threshold': 250, 'speech threshold': 120})),
    ("16 kHz, 320 / 160 samples, forget factor 100",
     dict(A.DEFAULT_CONFIG, **{'sample rate': 16000, 'forget factor': 100, 'adjustment': 0.02, 'onset threshold': 4,
                               'offset threshold': 0.5, 'silence threshold': 300, 'speech threshold': 100, 'start boundary': 100})),
]
N_STREAMS = 29
N_RECORDINGS = 24


def burst_signal(rng, n, sigma, bursts, amp=4000.0, freq=440.0, rate=8000):
    """test_gpu_audio_capture.burst_signal (the same lines: that module needs the golden files at import)."""
    t = np.arange(n) / rate
    x = rng.normal(0.0, sigma, size=n) if sigma > 0 else np.zeros(n)
    for a, b in bursts:
        x[a:b] += amp * np.sin(2 * np.pi * freq * t[a:b])
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def recordings(raw, seed):
    """(signals, ids): N_RECORDINGS seeded burst signals of 0 .. 3.5 s at the config's rate -- among them an empty one, one
    shorter than a frame, one shorter than 11 frames, one with three bursts, one still open at its end, one clipped to full
    scale, two under 0.2 s -- and the distinct stream ids (scattered over N_STREAMS) they are placed on."""
    rng = np.random.default_rng(seed)
    rate = raw['sample rate']
    cfg = A.derive(raw)
    width, stride = cfg['samples per frame'], cfg['frame stride']
    sigs = []
    for i in range(N_RECORDINGS):
        n = int(rng.integers(0, int(3.5 * rate)))
        bursts = []
        for _ in range(int(rng.integers(0, 4))):
            if n > 10:
                a = int(rng.integers(0, n))
                bursts.append((a, min(n, a + int(rng.integers(rate // 20, rate)))))
        sigma = 0.0 if i % 10 == 7 else float(rng.uniform(0.3, 300))
        sigs.append(burst_signal(rng, n, sigma, bursts, amp=float(rng.uniform(200, 12000)), freq=float(rng.uniform(100, 2000)), rate=rate))
    sigs[0] = np.zeros(0, dtype=np.int16)
    sigs[1] = burst_signal(rng, width - 1, 50, [], rate=rate)
    sigs[2] = burst_signal(rng, 6 * stride + width + 3, 50, [(stride, 4 * stride)], rate=rate)
    r10 = rate // 10                                       # bursts of 0.4 s, 0.65 s apart: longer than every config's silence threshold
    sigs[3] = burst_signal(rng, 35 * r10, 50, [(3 * r10, 7 * r10), (27 * r10 // 2, 35 * r10 // 2), (24 * r10, 28 * r10)], rate=rate)
    sigs[4] = burst_signal(rng, 2 * rate, 50, [(rate, 2 * rate)], rate=rate)                  # speech runs to the end: open
    sigs[5] = burst_signal(rng, 2 * rate, 50, [(rate // 2, rate)], amp=400000.0, rate=rate)   # clipped to full scale
    sigs[6] = burst_signal(rng, int(0.19 * rate), 80, [(rate // 50, rate // 10)], rate=rate)  # the two fed sample by sample
    sigs[8] = burst_signal(rng, int(0.12 * rate) + 1, 20, [], rate=rate)
    ids = np.random.default_rng(seed + 1).permutation(N_STREAMS)[:N_RECORDINGS]
    return sigs, [int(k) for k in ids]


SAMPLE_BY_SAMPLE = (6, 8)


def cuttings(rng, n, width, stride, index):
    """name -> chunk lengths (they sum to n; zeros are ticks the stream sits out) for recording `index` of `recordings`."""
    def ticks(c):
        return [min(c, n - k) for k in range(0, n, c)]
    choice = [0, 1, stride - 1, stride, width - 1, width, width + 1, 2 * width + 3, 5000]
    rand = []
    while sum(rand) < n:
        rand.append(int(min(choice[int(rng.integers(0, len(choice)))], n - sum(rand))))
    out = {"whole": [n], "width": ticks(width), "1024": ticks(1024), "random": rand}
    if index in SAMPLE_BY_SAMPLE:
        out["one"] = [1] * n
    return out
