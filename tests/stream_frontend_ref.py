# -*- coding: utf-8 -*-
"""Host restatements of the streaming front-end for the tests (numpy only, no GPU):

* `frames_ready_brute`: the contract spelled out frame by frame -- frame t is complete iff t * step + flen <= n, pairs
  (2m, 2m + 1) are computed when both are complete, a feature frame needs the cepstra two frames ahead;
* `CarriedStack`: the stack kernel's bookkeeping -- cepstral rows arrive in groups, the last 4 are carried at r & 3, every
  call emits the rows [ceps | delta | delta-delta] that became final (all of them once the end flag is set);
* `FakeStreamFrontend`: a double of `_hip.StreamFrontend` on the oracle's MFCC and `CarriedStack`, which returns
  `fake_hip.Batch` objects -- for the host logic of `StreamingFrontend` and `OnlineDecoder.push_audio`."""
import numpy as np

import fake_hip
from oracle import ref_numpy as O


def frames_ready_brute(n, flen, step, ended=False):
    if ended:
        return -(-n // step)
    complete = 0
    while complete * step + flen <= n:                    # frames 0 .. complete - 1 have all their samples
        complete += 1
    computed = complete - complete % 2                    # whole pairs only
    return max(0, computed - 2)                           # delta-delta of frame t reads cepstra t + 2


def raw_stack(ceps):
    """[ceps | delta | delta-delta] without the standardisation (core.py:27-29)."""
    d = O.delta_feature(ceps)
    return np.concatenate([ceps, d, O.delta_feature(d)], axis=1)


class CarriedStack:
    """Rows of one utterance's cepstra [T, C] arrive in groups; `push(rows, end)` returns the stacked rows that became
    final.  Only the last 4 cepstral rows are kept between calls, row r in slot r & 3."""

    def __init__(self, C):
        self.C = C
        self.keep = np.full((4, C), np.nan)
        self.have = 0                                     # cepstral rows seen
        self.done = 0                                     # stacked rows emitted

    def push(self, rows, end=False):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, self.C)
        first, last = self.have, self.have + len(rows)
        T = last if end else None
        if end and T < 2:
            raise IndexError("index 1 is out of bounds for axis 0 with size %d" % T)

        def f(r):
            assert first - 4 <= r < last and r >= 0, "row %d is neither new nor carried" % r
            return rows[r - first] if r >= first else self.keep[r & 3]

        def delta(t):
            if t == 0:
                return f(1) - f(0)
            if T is not None and t == T - 1:
                return f(t) - f(t - 1)
            return f(t + 1) - f(t - 1)

        stop = T if end else max(0, last - 2)
        out = []
        for t in range(self.done, stop):
            d = delta(t)
            if t == 0:
                dd = delta(1) - d
            elif T is not None and t == T - 1:
                dd = d - delta(t - 1)
            else:
                dd = delta(t + 1) - delta(t - 1)
            out.append(np.concatenate([f(t), d, dd]))
        for r in range(max(first, last - 4), last):
            self.keep[r & 3] = rows[r - first]
        self.have, self.done = last, max(self.done, stop)
        return np.array(out).reshape(-1, 3 * self.C)


class FakeStreamFrontend:
    """`_hip.StreamFrontend` on the host: keeps every stream's audio, computes the utterance's cepstra so far with the
    oracle (`O.mfcc_features_signal` on the samples received, complete frames only) and stacks them with `CarriedStack`.
    Like the real one it trusts its caller's checks and asserts them."""
    pushes = 0

    def __init__(self, ctx, n_streams, sample_rate=16000, mfcc_params=None, max_chunk=16000, dtype=np.float64, normalize=None):
        fs, st, lo, hi = mfcc_params if mfcc_params is not None else (0.025, 0.01, 80, None)
        self.ctx, self.n_streams, self.rate, self.prm = ctx, int(n_streams), int(sample_rate), (fs, st, lo, hi)
        self.flen, self.step = int(fs * self.rate), int(st * self.rate)
        self.max_chunk, self.np_dtype, self.normalize = int(max_chunk), np.dtype(dtype), normalize
        self.reset()

    def reset(self, ids=None):
        if ids is None:
            self.pcm = [np.zeros(0, dtype=np.int16) for _ in range(self.n_streams)]
            self.stack = [CarriedStack(13) for _ in range(self.n_streams)]
            self.over = [False] * self.n_streams
            return
        for k in ids:
            self.pcm[int(k)], self.stack[int(k)], self.over[int(k)] = np.zeros(0, dtype=np.int16), CarriedStack(13), False

    def samples(self):
        return np.array([len(x) for x in self.pcm], dtype=np.int64)

    def push(self, ids, samples, sample_off, end=None):
        type(self).pushes += 1
        ids = np.asarray(ids, dtype=np.int64)
        assert samples.dtype == np.int16 and len(sample_off) == len(ids) + 1 and len(set(ids.tolist())) == len(ids)
        assert len(ids) == 0 or (ids.min() >= 0 and ids.max() < self.n_streams)
        out = []
        for u, k in enumerate(ids):
            chunk = samples[sample_off[u]:sample_off[u + 1]]
            fin = bool(end is not None and end[u])
            assert len(chunk) <= self.max_chunk and not self.over[k]
            self.pcm[k] = np.concatenate([self.pcm[k], chunk])
            n = len(self.pcm[k])
            if fin:
                have = -(-n // self.step)
                assert have >= 2
            else:
                complete = 0 if n < self.flen else (n - self.flen) // self.step + 1
                have = complete - complete % 2            # cepstra exist for whole pairs of complete frames
            st = self.stack[k]
            if have > st.have:
                # complete frames do not depend on the audio behind them: the oracle on the prefix gives their cepstra
                ceps = O.mfcc_features_signal(self.pcm[k], self.rate, *self.prm)[1][st.have:have]
            else:
                ceps = np.zeros((0, 13))
            x = st.push(ceps, end=fin)
            if self.normalize is not None:
                x = (x - self.normalize[0]) / self.normalize[1]
            self.over[k] = fin
            out.append(x.astype(self.np_dtype))
        return fake_hip.Batch(self.ctx, out, dtype=self.np_dtype)

    def close(self):
        pass
