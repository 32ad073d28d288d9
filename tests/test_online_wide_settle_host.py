# -*- coding: utf-8 -*-
"""The settled prefix of an online decode of MORE THAN 16 WORDS, on the host (no GPU).

1. The bit-level restatement of the wide session (tests/online_wide_settle_ref.py: the wide sweep's decision words in a
   ring of columns, a mask of live states per lane, the loop-row hop as two 64-bit ballots and the lowest set lane, the
   set size from two ballots, the segment walk's label rule) against `online_settle_ref.SettledDecode` on
   `online_ref.CarriedDecode`, which walk graph rows and back-pointers: the carried column, the anchor (column, row) and
   the settled words at every tick, on `O.loop_grammar` graphs of (W, n, skip) = (17, 3, no), (20, 4, yes), (64, 2, no)
   fed in chunks of 0 .. 4 frames.  This pins the bit layout and the lowest-lane rule without a GPU.
2. The routing of `sr.recognition.batch.OnlineDecoder` on test doubles: a decoder of more than 16 words with settle=True
   makes the wide session class with `settle=True` (max_frames=) or `window=`; without settle it makes the
   four-positional call of before and refuses `window=` with no session made; a 16-word decoder routes as without
   settle.  commit / settled / settled_times / reset / finish bookkeeping; a push that overruns the window raises
   ValueError and reaches no backend.  The decoder that does not settle is pinned by tests/test_online_wide_host.py.
3. The ABI entry is in the header, in the ctypes table and in the library."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fake_hip
from conftest import ROOT
from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from online_wide_settle_ref import WideSettle, WideSweep
from oracle import ref_numpy as O
from test_online_host import word_trans
from test_online_wide_host import D_, FakeLoopSession, make_models


def favoured_emissions(rng, nes, rw, rs, W, n, T):
    """Emissions that favour a word sequence: without them nothing separates the words and nothing settles."""
    E = np.where(nes[:, None], 0.0, rng.uniform(3.0, 9.0, size=(len(nes), T)))
    t = 0
    while t < T:
        wd, Tw = int(rng.integers(0, W)), int(rng.integers(n, 2 * n + 3))
        for k in range(min(Tw, T - t)):
            E[np.flatnonzero((rw == wd) & (rs == min(k * n // Tw, n - 1)))[0], t + k] = rng.uniform(0.1, 0.6)
        t += Tw
    return E


@pytest.mark.parametrize("W,n,skip", [(17, 3, False), (20, 4, True), (64, 2, False)])
def test_bit_level_restatement_equals_the_row_level_one(W, n, skip):
    rng = np.random.default_rng(6400 + 10 * W + n)
    nes, rw, rs, trans, ends = O.loop_grammar([word_trans(rng, n, skip) for _ in range(W)], n, float(rng.choice([0.0, 0.7])))
    T = 60
    E = favoured_emissions(rng, nes, rw, rs, W, n, T)
    chunks = []
    while sum(chunks) < T:
        chunks.append(min(int(rng.integers(0, 5)), T - sum(chunks)))
    assert 0 in chunks and 4 in chunks
    # the row-level restatement first: it also says how long the ring has to be
    cd = CarriedDecode(nes, trans, ends)
    sd = SettledDecode(cd, rw)
    t, ref = 0, []
    for c in chunks:
        cd.push(E[:, t:t + c])
        t += c
        tail = t - sd.settled_frames
        new = sd.commit()
        ref.append((sd.anchor, list(sd.words), new, tail, cd.col.copy()))
    ring_cols = max(r[3] for r in ref) + 1
    assert ring_cols < T // 2, "the ring must wrap"
    sw = WideSweep(trans, W, n, ring_cols=ring_cols)
    assert sw.skip == skip and sw.hb == n + 2 + (n - 2 if skip else 0)
    ws = WideSettle(sw)
    t, advanced = 0, 0
    for c, (anchor, words, new, tail, col) in zip(chunks, ref):
        sw.push(E[:, t:t + c])
        t += c
        if t:
            np.testing.assert_array_equal(sw.prev[:, :W], col[sw.row])    # the carried column, bitwise
        before = ws.anchor
        assert ws.commit() == new and ws.words == words and ws.flag == 0
        assert (None if ws.anchor is None else (ws.anchor[0], ws.row_of(ws.anchor[1], ws.anchor[2]))) == anchor
        advanced += ws.anchor != before
    assert advanced >= 3 and len(ws.words) >= 3 and len(ws.passed) >= 3     # not vacuous: anchors move, walks hop


# ----------------------------------------------------------------------------------------------------------------------
class FakeWideSettleSession(FakeLoopSession):
    """Test double of `_hip.OnlineWideSession` with the opt-in: the parent double's carried recursion, plus commit / tail
    on the row-level restatement and the window check of a push.  It records how it was constructed."""
    how = []                                          # (number of positional arguments, keywords) of every construction
    calls = 0                                         # calls that reached the backend

    def __init__(self, *args, **kw):
        type(self).how.append((len(args), dict(kw)))
        p = dict(zip(("ctx", "lat", "n_streams", "max_frames", "window", "settle"), args), **kw)
        max_frames, window = p.get("max_frames"), p.get("window")
        assert (max_frames is None) != (window is None)
        super().__init__(p["ctx"], p["lat"], p["n_streams"], 1 << 40 if max_frames is None else max_frames)
        self.window = window
        self.settles = bool(p.get("settle", False)) or window is not None
        self.sd = [None] * self.n_streams
        self.n_settled = [0] * self.n_streams

    def push(self, batch, ids, first=None, count=None):
        type(self).calls += 1
        if self.window is not None:
            idx = np.asarray(ids, dtype=np.int64)
            f = np.zeros(batch.U, dtype=np.int64) if first is None else np.asarray(first)
            c = batch.lengths - f if count is None else np.asarray(count)
            settled = np.array([0 if self.sd[k] is None else self.sd[k].settled_frames for k in idx])
            assert np.all(self.frames()[idx] + c - settled <= self.window)
        super().push(batch, ids, first, count)

    def reset(self, ids=None):
        super().reset(ids)
        for k in (range(self.n_streams) if ids is None else ids):
            self.sd[int(k)], self.n_settled[int(k)] = None, 0

    def result(self, ids=None, row_label=None, max_labels=None, want_path=False, want_begin=False):
        from sr.recognition import _hip
        if self.window is not None:
            raise _hip.Unsupported("a session with a window: tail()")
        return super().result(ids, row_label, max_labels, want_path, want_begin)

    def commit(self, ids=None, row_label=None, max_labels=None, want_begin=False):
        from sr.recognition import _hip
        from sr.recognition.batch import path_to_word_times
        if not self.settles:
            raise _hip.Unsupported("a wide session does not settle")
        type(self).calls += 1
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        assert len(set(ids.tolist())) == len(ids)
        rl = np.asarray(row_label)
        labels, begins = [], []
        for k in (int(v) for v in ids):
            if self.sd[k] is None:
                self.sd[k] = SettledDecode(self.streams[k], rl)
            sd = self.sd[k]
            new = sd.commit()
            wds, bgs = path_to_word_times(sd.path_from(sd.anchor[1], sd.anchor[0]), np.where(rl < 0, -1, rl), 1) if sd.anchor is not None else ([], [])
            assert wds == sd.words and wds[self.n_settled[k]:] == new
            labels.append(np.array(new, dtype=np.int32))
            begins.append(np.array(bgs[self.n_settled[k]:], dtype=np.int32))
            self.n_settled[k] = len(wds)
        out = dict(settled_frames=np.array([self.sd[int(k)].settled_frames for k in ids], dtype=np.int64), labels=labels)
        if want_begin:
            out["begins"] = begins
        return out

    def tail(self, ids=None, row_label=None, max_labels=None, want_begin=False):
        from sr.recognition import _hip
        if not self.settles:
            raise _hip.Unsupported("a wide session does not settle")
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        out = FakeLoopSession.result(self, ids, row_label, max_labels, False, want_begin)
        if row_label is not None:
            for i, k in enumerate(int(v) for v in ids):
                C = [] if self.sd[k] is None else self.sd[k].words
                assert out["labels"][i].tolist()[:len(C)] == C
                out["labels"][i] = out["labels"][i][len(C):]
                if want_begin:
                    out["begins"][i] = out["begins"][i][len(C):]
        return out


class FakeNarrow(FakeWideSettleSession):
    pass


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", FakeNarrow, raising=False)
    monkeypatch.setattr(_hip, "OnlineWideSession", FakeWideSettleSession, raising=False)
    monkeypatch.setattr(FakeWideSettleSession, "how", [])
    monkeypatch.setattr(FakeWideSettleSession, "calls", 0)
    monkeypatch.setattr(FakeLoopSession, "made", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def test_routing_of_a_wide_and_of_a_narrow_decoder(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(61)
    hmms, _ = make_models(rng, 17)
    dec = ContinuousDecoder(hmms, grammar="loop")
    how = FakeWideSettleSession.how
    on = dec.online(2, max_frames=9, settle=True)
    assert type(on.session) is FakeWideSettleSession and on.wide and on.settles and on.max_frames == 9 and on.window is None
    assert how[-1] == (4, dict(settle=True))
    on = dec.online(2, window=7, settle=True)
    assert type(on.session) is FakeWideSettleSession and on.wide and on.settles and on.window == 7 and on.max_frames is None
    assert how[-1] == (3, dict(window=7))
    on = dec.online(2, max_frames=9)                                       # without settle: the four positional arguments of before
    assert type(on.session) is FakeWideSettleSession and on.wide and not on.settles and how[-1] == (4, {})
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(_hip.Unsupported):
            call([0])
    made = len(how)
    for kw in (dict(window=7), dict(window=7, settle=False)):
        with pytest.raises(_hip.Unsupported):
            dec.online(2, **kw)
    for kw in (dict(settle=True), dict(max_frames=5, window=5, settle=True), dict(window=0, settle=True), dict(max_frames=0, settle=True)):
        with pytest.raises(ValueError):
            dec.online(2, **kw)
    assert len(how) == made                                                # refused before a session is made
    # 16 words: settle changes nothing, the narrow class is asked as ever
    hmms16, _ = make_models(rng, 16)
    dec16 = ContinuousDecoder(hmms16, grammar="loop")
    for settle in (False, True):
        on = dec16.online(2, max_frames=9, settle=settle)
        assert type(on.session) is FakeNarrow and not on.wide and on.settles and how[-1] == (4, {})
        on = dec16.online(2, window=7, settle=settle)
        assert type(on.session) is FakeNarrow and how[-1] == (3, dict(window=7))


@pytest.mark.parametrize("windowed", [False, True])
def test_wide_opt_in_commit_settled_result_and_times(fake_backend, windowed):
    """Interleaved pushes and commits on a 19-word decoder with times=True: `settled` / `settled_times` grow by what
    `commit(want_times=True)` returns, `result` is settled + tail and equals the carried decode of the prefix (words and
    begins), `finish` frees an id and it decodes a fresh utterance -- with full history and with a window far shorter
    than the streams."""
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder, path_to_word_times
    rng = np.random.default_rng(62)
    W = 19
    hmms, utterance = make_models(rng, W)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=0.4)
    g = dec.lat.graphs[0]
    nes = np.asarray(g["row_state"]) < 0
    WINDOW = 40
    utts = {k: utterance(rng.integers(0, W, size=int(rng.integers(18, 22)))) for k in range(3)}
    assert min(len(x) for x in utts.values()) >= 2 * WINDOW
    on = dec.online(3, window=WINDOW, settle=True, times=True) if windowed else \
        dec.online(3, max_frames=max(len(x) for x in utts.values()), settle=True, times=True)
    assert on.settled()[0] == [[]] * 3 and on.commit() == [[]] * 3 and on.result()[0] == [[]] * 3
    pos = {k: 0 for k in utts}
    reused = False
    for tick in range(400):
        live = [k for k in utts if pos[k] < len(utts[k])]
        if not live:
            break
        ids = [int(k) for k in rng.permutation(live)[:rng.integers(1, len(live) + 1)]]
        lens = [int(rng.integers(0, 6)) for _ in ids]
        on.push(ids, [utts[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)])
        for k, c in zip(ids, lens):
            pos[k] = min(pos[k] + c, len(utts[k]))
        (before, before_frames), before_t = on.settled(ids), on.settled_times(ids)
        if tick % 2:
            new, new_t = on.commit(ids, want_times=True)
        else:
            new, new_t = on.commit(ids), None
        (after, after_frames), after_t = on.settled(ids), on.settled_times(ids)
        assert after == [b + n for b, n in zip(before, new)] and np.all(after_frames >= before_frames)
        assert np.all(after_frames <= np.maximum(on.frames[ids] - 1, 0))
        assert [len(a) for a in after_t] == [len(a) for a in after]
        if new_t is not None:
            assert after_t == [b + n for b, n in zip(before_t, new_t)]
        done = [k for k in ids if pos[k] == len(utts[k])]
        if tick % 15 == 0 or done:                                         # (the double decodes the whole prefix: not every tick)
            some = [k for k in ids if pos[k] >= 2]
            if some:
                b = _hip.Batch(dec.ctx, [utts[k][:pos[k]] for k in some])
                b.loglik(dec.gmm, fetch=False)
                got, info = on.result(some)
                assert info["frames"].tolist() == [pos[k] for k in some]
                for u, k in enumerate(some):
                    cd = CarriedDecode(nes, dec.lat._dense(g), g["end_rows"])
                    cd.push(dec.lat._emissions(b, u, g)[0])
                    rw_, rb = path_to_word_times(cd.result()[2], dec.row_state, dec.n)
                    assert got[u] == rw_ and info["begins"][u].tolist() == rb
                    C, Ct = on.settled([k])[0][0], on.settled_times([k])[0]
                    assert C == rw_[:len(C)] and Ct == rb[:len(C)]
        if done and not reused:
            k = done[0]
            assert len(on.settled([k])[0][0]) >= 3                         # words were final long before the end
            on.finish([k])
            assert on.frames[k] == 0 and on.settled([k])[0] == [[]] and on.settled([k])[1].tolist() == [0]
            assert on.settled_times([k]) == [[]]
            utts[k], pos[k], reused = utterance([18, 2, 17, 3, 16, 0]), 0, True   # the id decodes a fresh utterance
    assert reused and all(pos[k] == len(utts[k]) for k in utts)
    assert all(len(w) >= 3 for w in on.settled()[0])
    if windowed:
        with pytest.raises(ValueError):
            on.result([0], want_path=True)
    else:
        assert len(on.result([0], want_path=True)[1]["paths"][0]) > 0      # full history keeps its paths
    on.reset()
    assert on.frames.tolist() == [0] * 3 and on.settled()[0] == [[]] * 3 and not on.settled()[1].any()
    assert on.settled_times() == [[]] * 3
    on.close()


def test_a_push_past_the_window_reaches_no_backend(fake_backend):
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(63)
    W = 18
    hmms, utterance = make_models(rng, W)
    dec = ContinuousDecoder(hmms, grammar="loop")
    WINDOW = 40
    on = dec.online(3, window=WINDOW, settle=True)
    x = utterance(rng.integers(0, W, size=30))
    assert len(x) >= 3 * WINDOW
    on.push([2, 0], [x[:WINDOW], x[:3]])                                  # exactly the window is fine
    frames, calls = on.frames, FakeWideSettleSession.calls
    assert frames.tolist() == [3, 0, WINDOW]
    for ids, chunks in (([1, 2], [x[:2], x[WINDOW:WINDOW + 1]]),          # stream 2: one frame too many -- stream 1 must not move
                        ([0], [x[3:WINDOW + 1]])):
        with pytest.raises(ValueError, match="stream %d" % ids[-1]):
            on.push(ids, chunks)
        assert on.frames.tolist() == frames.tolist() and FakeWideSettleSession.calls == calls
    for bad in ([1, 1], [3], [-1]):
        with pytest.raises(ValueError):
            on.commit(bad)
        assert FakeWideSettleSession.calls == calls
    with pytest.raises(ValueError):
        on.commit([0], want_times=True)                                   # a decoder without times
    with pytest.raises(ValueError):
        on.finish([2], want_path=True)
    assert on.frames.tolist() == frames.tolist()
    pos = WINDOW                                                          # a commit moves the window on
    while pos < len(x):
        on.commit([2])
        room = WINDOW - (on.frames[2] - on.settled([2])[1][0])
        assert room > 0, "the traces of this stream meet within the window"
        on.push([2], [x[pos:pos + room]])
        pos = min(pos + room, len(x))
    assert on.frames[2] == len(x)
    on.commit([2])
    C = on.settled([2])[0][0]
    assert len(C) >= 2 and on.result([2])[0][0][:len(C)] == C
    on.reset([2])
    assert on.settled([2])[1].tolist() == [0]
    on.push([2], [x[:WINDOW]])
    assert on.frames.tolist() == [3, 0, WINDOW]
    with pytest.raises(ValueError):
        on.push([1], [rng.normal(size=(4, D_ + 1))])
    on.close()


def test_header_binding_and_library_have_the_entry(built_library):
    from sr.recognition import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmmhmm.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gh_online_create_wide_settle\s*\(", text)
    assert _hip.SIGNATURES["gh_online_create_wide_settle"] == _hip.SIGNATURES["gh_online_create_bigram_settle"]
    assert hasattr(ctypes.CDLL(built_library), "gh_online_create_wide_settle")
    assert list(inspect.signature(_hip.OnlineWideSession.__init__).parameters)[1:] == ["ctx", "lat", "n_streams", "max_frames", "window", "settle"]
