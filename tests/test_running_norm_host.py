# -*- coding: utf-8 -*-
"""The causal running mean / variance normalisation on the host (no GPU).

1. The numpy restatement (tests/running_norm_ref.py) against the rule's two limits -- prior_frames = 0: the last frame is
   the last row of the reference's `standardize`; prior_frames huge: the fixed map -- the floor, the one-frame utterance,
   and the carried state: normalising x[:k] then x[k:] equals normalising x, for every k, bitwise.
2. `RunningNorm` refuses every bad argument with ValueError.
3. Routing on test doubles defined here: which backend constructor `StreamingFrontend` calls with which arguments, `reset`
   against `reset_stats` under both `per` values, `features_from_signals` -> `Batch.running_norm`; a pair / None still
   takes the old constructor and `Batch.affine`.
4. `_OnlineStreams.reset` calls `reset_stats`, `_reset_utterance` does not.
5. The built library exports the four new symbols and the binding declares them."""
import ctypes

import numpy as np
import pytest

from oracle import ref_numpy as O
from running_norm_ref import running_norm

D = 39


def utterance(rng, T, dim=D):
    return rng.normal(size=(T, dim)) * rng.uniform(1.0, 6.0, size=dim) + rng.normal(size=dim) * 3.0


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("T", [2, 3, 50])
def test_without_a_prior_the_last_row_is_standardize(T):
    rng = np.random.default_rng(230 + T)
    x = utterance(rng, T)
    mean, std = rng.normal(size=D), rng.uniform(0.5, 2.0, size=D)
    y, (S, Q, c) = running_norm(x, mean, std, prior_frames=0, min_std=1e-6)
    assert c == T
    np.testing.assert_allclose(y[-1], O.standardize(x.copy())[-1], rtol=1e-9, atol=1e-9)


def test_a_heavy_prior_is_the_fixed_map():
    rng = np.random.default_rng(231)
    x = utterance(rng, 50)
    mean, std = rng.normal(size=D), rng.uniform(0.5, 2.0, size=D)
    y, _ = running_norm(x, mean, std, prior_frames=1e12)
    np.testing.assert_allclose(y, (x - mean) / std, rtol=1e-6, atol=1e-6)


def test_a_constant_coefficient_hits_the_floor_and_stays_finite():
    rng = np.random.default_rng(232)
    x = utterance(rng, 30)
    x[:, 7] = 4.25
    mean, std = np.zeros(D), np.ones(D)
    for P in (0, 1, 100):
        y, _ = running_norm(x, mean, std, prior_frames=P, min_std=0.1)
        assert np.all(np.isfinite(y))
        if P == 0:                                         # mean = the value, variance 0: the floor divides a zero
            np.testing.assert_array_equal(y[:, 7], 0.0)


def test_one_frame_without_a_prior_is_all_zeros():
    rng = np.random.default_rng(233)
    for dtype in (np.float64, np.float32):
        y, (S, Q, c) = running_norm(utterance(rng, 1), rng.normal(size=D), np.ones(D), prior_frames=0, dtype=dtype)
        assert c == 1 and y.dtype == dtype
        np.testing.assert_array_equal(y, np.zeros((1, D)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_carried_state_is_cutting_invariant(dtype):
    rng = np.random.default_rng(234)
    x = utterance(rng, 23)
    mean, std = rng.normal(size=D), rng.uniform(0.5, 2.0, size=D)
    whole, (S, Q, c) = running_norm(x, mean, std, prior_frames=5, dtype=dtype)
    for k in range(len(x) + 1):
        head, st = running_norm(x[:k], mean, std, prior_frames=5, dtype=dtype)
        assert st[2] == k
        tail, st2 = running_norm(x[k:], mean, std, prior_frames=5, dtype=dtype, state=st)
        np.testing.assert_array_equal(np.concatenate([head, tail]), whole)
        np.testing.assert_array_equal(st2[0], S)
        np.testing.assert_array_equal(st2[1], Q)
        assert st2[2] == c == len(x)


# ------------------------------------------------------------------ 2. the value object
def test_running_norm_refuses_bad_arguments():
    from sr.feature import RunningNorm
    m, s = np.zeros(D), np.ones(D)
    ok = RunningNorm((m, s))
    assert (ok.prior_frames, ok.min_std, ok.per) == (100.0, 0.1, "utterance")
    assert RunningNorm((m, s), 0, 1.0, "stream").per == "stream"
    bad_s, nan_m, inf_s, neg_s = s.copy(), m.copy(), s.copy(), s.copy()
    bad_s[3], nan_m[0], inf_s[38], neg_s[5] = 0.0, np.nan, np.inf, -1.0
    for args, kw in ((((m, bad_s),), {}), (((nan_m, s),), {}), (((m, inf_s),), {}), (((m, neg_s),), {}),
                     (((m[:13], s[:13]),), {}), (((m, s[:13]),), {}), ((m,), {}), ((None,), {}),
                     (((m, s),), dict(prior_frames=-1)), (((m, s),), dict(prior_frames=2.5)),
                     (((m, s),), dict(prior_frames=np.inf)), (((m, s),), dict(prior_frames=np.nan)),
                     (((m, s),), dict(prior_frames="many")),
                     (((m, s),), dict(min_std=0.0)), (((m, s),), dict(min_std=-0.1)), (((m, s),), dict(min_std=1.5)),
                     (((m, s),), dict(min_std=np.nan)),
                     (((m, s),), dict(per="speaker")), (((m, s),), dict(per=None))):
        with pytest.raises(ValueError):
            RunningNorm(*args, **kw)


# ------------------------------------------------------------------ 3. routing on test doubles
class FakeBatch:
    """Stands for `_hip.Batch`: records how it was made and what was applied to it."""
    made = []

    def __init__(self, ctx, utterances=None, **kw):
        self.ctx, self.kw, self.applied = ctx, kw, []
        self.lengths = np.zeros(0, dtype=np.int64)
        FakeBatch.made.append(self)

    def affine(self, mean, std):
        self.applied.append(("affine", mean, std))
        return self

    def running_norm(self, mean, std, prior_frames, min_std):
        self.applied.append(("running_norm", mean, std, prior_frames, min_std))
        return self


class FakeFixedBackend:
    """Stands for `_hip.StreamFrontend`: the old constructor."""
    made = []

    def __init__(self, *args, **kw):
        assert not kw
        self.args, self.calls = args, []
        type(self).made.append(self)

    def push(self, ids, pcm, off, end):
        self.calls.append(("push", list(ids)))
        b = FakeBatch.__new__(FakeBatch)
        b.lengths = self.counts
        return b

    def reset(self, ids):
        self.calls.append(("reset", None if ids is None else list(ids)))

    def close(self):
        pass


class FakeRunningBackend(FakeFixedBackend):
    """Stands for `_hip.RunningStreamFrontend`."""
    made = []

    def reset_stats(self, ids):
        self.calls.append(("reset_stats", None if ids is None else list(ids)))


@pytest.fixture
def doubles(monkeypatch, built_library):
    from sr.recognition import _hip
    ctx = object()
    monkeypatch.setattr(_hip, "default_context", lambda device=None: ctx)
    monkeypatch.setattr(_hip, "Batch", FakeBatch)
    monkeypatch.setattr(_hip, "StreamFrontend", FakeFixedBackend)
    monkeypatch.setattr(_hip, "RunningStreamFrontend", FakeRunningBackend, raising=False)
    for cls in (FakeBatch, FakeFixedBackend, FakeRunningBackend):
        monkeypatch.setattr(cls, "made", [])
    return ctx


def test_streaming_frontend_routes_a_running_norm(doubles):
    from sr.feature import RunningNorm, StreamingFrontend
    m, s = np.arange(D, dtype=np.float64), np.arange(D, dtype=np.float64) + 1.0
    for per, keep in (("utterance", False), ("stream", True)):
        norm = RunningNorm((m, s), prior_frames=40, min_std=0.25, per=per)
        fe = StreamingFrontend(3, 8000, normalize=norm, max_chunk=700, dtype=np.float32, low_freq=60)
        assert not FakeFixedBackend.made and len(FakeRunningBackend.made) == 1
        be = FakeRunningBackend.made.pop()
        assert fe.backend is be and fe.D == 39
        ctx, n, rate, prm, max_chunk, dtype, prior, pf, ms, k = be.args
        assert (ctx, n, rate, max_chunk, dtype, pf, ms, k) == (doubles, 3, 8000, 700, np.dtype(np.float32), 40.0, 0.25, keep)
        assert prm == (0.025, 0.01, 60, None)
        np.testing.assert_array_equal(prior[0], m)
        np.testing.assert_array_equal(prior[1], s)
        # frames advance the count of the statistics where samples advance
        assert fe.norm_frames.tolist() == [0, 0, 0]
        x = np.zeros(700, dtype=np.int16)                  # 8 kHz: frames of 200 every 80 -> 7 complete, 6 computed, 4 final
        be.counts = np.array([4, 0])
        fe.push([2, 0], [x, x[:100]])
        assert fe.norm_frames.tolist() == [0, 0, 4] and fe.samples.tolist() == [100, 0, 700]
        with pytest.raises(ValueError):
            fe.push([1, 1], [x, x])                        # refused: nothing moves
        with pytest.raises(ValueError):
            fe.push([1], [np.zeros(701, dtype=np.int16)])
        assert fe.norm_frames.tolist() == [0, 0, 4] and fe.samples.tolist() == [100, 0, 700]
        # reset against reset_stats
        fe.reset([2])
        assert fe.samples.tolist() == [100, 0, 0]
        assert fe.norm_frames.tolist() == ([0, 0, 4] if keep else [0, 0, 0])
        assert be.calls == [("push", [2, 0]), ("reset", [2])]          # (the library clears its own count under per="utterance")
        fe.reset_stats([2])
        assert fe.norm_frames.tolist() == [0, 0, 0] and be.calls[-1] == ("reset_stats", [2])
        fe.reset_stats()
        assert be.calls[-1] == ("reset_stats", None)
        with pytest.raises(ValueError):
            fe.reset_stats([3])


def test_a_pair_or_none_takes_the_old_constructor(doubles):
    from sr.feature import StreamingFrontend
    m, s = np.zeros(D), np.ones(D)
    for normalize in (None, (m, s)):
        fe = StreamingFrontend(2, normalize=normalize, max_chunk=500)
        assert not FakeRunningBackend.made and len(FakeFixedBackend.made) == 1
        be = FakeFixedBackend.made.pop()
        ctx, n, rate, prm, max_chunk, dtype, norm = be.args
        assert (ctx, n, rate, prm, max_chunk, dtype) == (doubles, 2, 16000, (0.025, 0.01, 80, None), 500, np.dtype(np.float64))
        assert (norm is None) if normalize is None else (np.array_equal(norm[0], m) and np.array_equal(norm[1], s))
        be.counts = np.array([0])
        fe.push([1], [np.zeros(300, dtype=np.int16)])
        fe.reset()
        fe.reset_stats()                                   # nothing to clear: the backend is not asked
        assert be.calls == [("push", [1]), ("reset", None)] and fe.norm_frames.tolist() == [0, 0]


def test_features_from_signals_routes_a_running_norm(doubles):
    from sr.feature import RunningNorm, features_from_signals
    m, s = np.arange(D, dtype=np.float64), np.ones(D)
    sigs = [np.zeros(800, dtype=np.int16)]
    b = features_from_signals(sigs, 16000, dtype=np.float32, normalize=RunningNorm((m, s), 7, 0.5, per="stream"))
    assert b is FakeBatch.made[-1] and b.kw["frontend_mode"] == 1 and b.kw["pcm"] is sigs and b.kw["dtype"] == np.float32
    (what, mean, std, pf, ms), = b.applied
    assert what == "running_norm" and (pf, ms) == (7.0, 0.5)
    np.testing.assert_array_equal(mean, m)
    np.testing.assert_array_equal(std, s)
    b = features_from_signals(sigs, 16000, normalize=(m, s))               # a pair: the fixed map, as ever
    assert [a[0] for a in b.applied] == ["affine"] and b.kw["frontend_mode"] == 1
    b = features_from_signals(sigs, 16000)                                 # None: per-utterance standardize, as ever
    assert b.applied == [] and "frontend_mode" not in b.kw


# ------------------------------------------------------------------ 4. the online decoders' reset
class Recorder:
    def __init__(self, *names):
        self.calls = []
        for name in names:
            setattr(self, name, (lambda nm: lambda ids=None: self.calls.append((nm, None if ids is None else list(ids))))(name))


def bare_streams(frontend):
    from sr.recognition.batch import _OnlineStreams
    on = _OnlineStreams.__new__(_OnlineStreams)
    on.session, on.frontend, on.endpointer = Recorder("reset"), frontend, Recorder("reset")
    on.n_streams, on._frames = 4, np.arange(4, dtype=np.int64) + 1
    return on


def test_online_reset_clears_the_statistics_and_the_utterance_reset_does_not():
    on = bare_streams(Recorder("reset", "reset_stats"))
    on._reset_utterance(np.array([1, 3]))
    assert on.frontend.calls == [("reset", [1, 3])] and on._frames.tolist() == [1, 0, 3, 0]
    on.reset([2])
    assert on.frontend.calls[1:] == [("reset", [2]), ("reset_stats", [2])]
    assert on.endpointer.calls == [("reset", [2])] and on.session.calls == [("reset", [1, 3]), ("reset", [2])]
    on.reset()
    assert on.frontend.calls[3:] == [("reset", None), ("reset_stats", None)] and on._frames.tolist() == [0, 0, 0, 0]
    # a front-end without statistics (a double of the old surface) and no front-end at all keep working
    old = bare_streams(Recorder("reset"))
    old.reset([0])
    assert old.frontend.calls == [("reset", [0])]
    none = bare_streams(None)
    none.reset()
    assert none._frames.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------ 5. the ABI
def test_the_library_exports_the_running_norm_entries(built_library):
    from sr.recognition import _hip
    lib = ctypes.CDLL(built_library)
    for name in ("gh_stream_create_running", "gh_stream_reset_stats", "gh_stream_norm_frames", "gh_batch_running_norm"):
        assert getattr(lib, name) is not None
        assert name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["gh_stream_create_running"][1]) == len(_hip.SIGNATURES["gh_stream_create"][1]) + 3
