# -*- coding: utf-8 -*-
"""The settled prefix of an online decode, on the host (no GPU).

DEFINITIONS.  L_k: the one-shot label list of the first k frames of a stream.  C: the settled words after a commit at T
frames.  A trace occupies, in a column, the cell in which it ARRIVES there coming from the column behind it (in a loop
grammar a path can hold three cells of one column: a first state, the loop row, the last state that fed it).

1. The restatement (tests/online_settle_ref.py) against brute force on `O.loop_grammar` graphs: at every tick, follow the
   back-pointers of EVERY finite emitting row of the newest column to column 0; the latest column <= T - 2 in which all
   those paths sit in one cell is the anchor, or there is none.  C == `O.path_to_words` of the path through the anchor, cut
   at the anchor; C == L_T[:len(C)]; C == L_m[:len(C)] for every later m.
   Streams whose end costs are all +inf are outside the stability contract (the one-shot back-trace then starts in a dead
   cell and follows the reference's arg-min over +inf costs, which need not pass the anchor): L_k is compared at the
   ticks at which the chosen end is finite, the anchor and C at every tick.
2. G14, the reference's own loop-grammar utterances, in chunks of 1, 5 and 50: the contract holds, and -- so that this
   cannot pass vacuously -- the two longer utterances (T = 29, 50) have an anchor at every tick from frame 15 on (frames
   counted from 0, like columns) at chunk 5, at most 13 frames behind the newest column.
3. The host logic of `OnlineDecoder.commit` / `settled` / `window=` on a double of the session: every refusal, reset /
   finish / id reuse, and a push that overruns the window moves nothing."""
import warnings

import numpy as np
import pytest

import fake_hip
from conftest import load_golden
from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from oracle import ref_numpy as O


def word_trans(rng, n, skip=False):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.05, 0.6) if i < n - 1 else rng.uniform(0.0, 0.3)
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.8, 2.5)
        if skip and i < n - 2 and rng.random() < 0.6:
            t[i + 2, i] = rng.uniform(1.5, 4.0)
    return t


def random_chunks(rng, T):
    """Chunk lengths 0 .. 4 that sum to T."""
    out = []
    while sum(out) < T:
        out.append(int(min(rng.integers(0, 5), T - sum(out))))
    if rng.random() < 0.5:
        out.append(0)
    return out


def one_shot_labels(E, nes, trans, ends, rw):
    """(L_k, cost of the chosen end) of the oracle's whole decode of the frames E."""
    if E.shape[1] == 0:
        return [], np.inf
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        costs, path = O.decode_states(E, nes, trans, end_points=[[e, E.shape[1] - 1] for e in ends])
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    return (O.path_to_words(path, nes, rw) if len(path) else []), float(np.min(costs[np.asarray(ends), -1]))


def brute_force_anchor(cd):
    """(column, row, the path from that cell to the start) of the latest column <= T - 2 in which the back-traces of all
    finite emitting rows of the newest column arrive in one cell; None if there is none."""
    T = cd.t
    if T < 2:
        return None
    arrivals = []                                                  # per live row: column -> (row, index into its path)
    paths = []
    for r in range(cd.R):
        if cd.is_nes[r] or not np.isfinite(cd.col[r]):
            continue
        i, j, path = r, T - 1, [[r, T - 1]]
        while j != 0:
            i, j = (int(v) for v in cd.bp[j][i])
            path.append([i, j])
        first = {}
        for k, (i, j) in enumerate(path):
            first.setdefault(j, (i, k))
        arrivals.append(first)
        paths.append(np.array(path, dtype=np.int64))
    for c in range(T - 2, -1, -1):
        cells = {a[c][0] for a in arrivals}
        if len(cells) == 1:
            row, k = arrivals[0][c]
            return c, row, paths[0][k:]
    return None


def run_contract(E, nes, rw, trans, ends, chunks):
    """Feeds E in `chunks`, commits after every chunk and checks the whole contract; returns per tick (T, anchor column
    or None)."""
    cd = CarriedDecode(nes, trans, ends)
    sd = SettledDecode(cd, rw)
    t, ticks, settled = 0, [], []
    for c in chunks:
        cd.push(E[:, t:t + c])
        t += c
        before = list(sd.words)
        new = sd.commit()
        assert sd.words == before + new                           # commits only ever extend
        bf = brute_force_anchor(cd)
        if bf is None:
            assert sd.anchor is None and sd.words == []
        else:
            assert sd.anchor == (bf[0], bf[1]) and bf[0] <= t - 2
            assert sd.words == O.path_to_words(bf[2], nes, rw)
        L, end_cost = one_shot_labels(E[:, :t], nes, trans, ends, rw)
        settled.append(list(sd.words))
        if np.isfinite(end_cost):
            for C in settled:                                      # this commit's C and every earlier one
                assert C == L[:len(C)]
        ticks.append((t, None if sd.anchor is None else sd.anchor[0]))
    assert t == E.shape[1]
    return ticks


@pytest.mark.parametrize("seed", range(24))
def test_restatement_equals_brute_force_and_the_prefix_is_stable(seed):
    rng = np.random.default_rng(9000 + seed)
    W, n = int(rng.integers(1, 6)), int(rng.integers(2, 7))
    skip = bool(seed % 2)
    nes, rw, rs, trans, ends = O.loop_grammar([word_trans(rng, n, skip) for _ in range(W)], n, float(rng.choice([0.0, 0.7, 2.5])))
    R = len(nes)
    T = int(rng.integers(1, 41)) if seed > 2 else seed + 1
    E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(R, T)))
    if seed % 5 == 0:
        E[rng.integers(1, R), rng.integers(0, T)] = np.inf            # an emission that underflowed
    run_contract(E, nes, rw, trans, ends, random_chunks(rng, T))


def test_some_restatement_cases_settle_words():
    """The parametrised test above is not vacuous: in a third of its cases a word is settled three frames before the end."""
    with_words = 0
    for seed in range(24):
        rng = np.random.default_rng(9000 + seed)
        W, n = int(rng.integers(1, 6)), int(rng.integers(2, 7))
        nes, rw, rs, trans, ends = O.loop_grammar([word_trans(rng, n, bool(seed % 2)) for _ in range(W)], n,
                                                  float(rng.choice([0.0, 0.7, 2.5])))
        T = int(rng.integers(1, 41)) if seed > 2 else seed + 1
        E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(len(nes), T)))
        cd = CarriedDecode(nes, trans, ends)
        sd = SettledDecode(cd, rw)
        cd.push(E[:, :max(T - 3, 0)])
        sd.commit()
        with_words += len(sd.words) >= 1
    assert with_words >= 8


def g14_ticks(chunk):
    """Per G14 utterance (both penalties): (T, [(frames, anchor column or None) per tick]), the contract checked on the way."""
    g = load_golden("G14_loop_grammar")
    means, vars_, w, wt = g["means"], g["vars"], g["w"], g["word_trans"]
    W, n = means.shape[:2]
    out = []
    for pen in (0, 1):
        pp = "p%d_" % pen
        nes, rw, rs, trans, ends = O.loop_grammar([wt] * W, n, float(g[pp + "penalty"]))
        states = [None if nes[r] else (means[rw[r], rs[r]], vars_[rw[r], rs[r]], w[rw[r], rs[r]]) for r in range(len(rw))]
        for u in range(int(g["n_utts"])):
            E = O.emission_matrix(g[pp + "x%d" % u], states)
            T = E.shape[1]
            out.append((T, run_contract(E, nes, rw, trans, ends, [min(chunk, T - t) for t in range(0, T, chunk)])))
    return out


@pytest.mark.parametrize("chunk", [1, 5, 50])
def test_G14_in_chunks(chunk):
    """The contract on the reference's own utterances; at chunk 5 every anchor is at most 13 frames behind the newest
    column (observed: 5 - 13), and the longer utterances do settle."""
    runs = g14_ticks(chunk)
    assert sorted(T for T, _ in runs) == [7, 7, 29, 29, 50, 50]
    if chunk == 5:
        for T, ticks in runs:
            lags = [(t - 1) - a for t, a in ticks if a is not None]
            assert all(lag <= 13 for lag in lags)
            assert T == 7 or len(lags) >= len(ticks) - 3


def test_G14_has_an_anchor_at_every_tick_from_frame_15_on():
    """Not vacuous: at chunk 5 the two longer utterances (T = 29, 50) have an anchor at every tick from frame 15 on, at most
    13 frames behind the newest column.  Frames are counted like columns, from 0: the ticks meant are those whose newest
    column is frame 15 or later, i.e. from 20 frames on (the tick of 15 frames ends with frame 14).  A property of the
    fixture: anchors per tick (frames taken: anchor column), penalty 0 -- penalty 1 differs at 30 frames only (18) --
    T = 29: 15: 8, 20: 12, 25: 12, 29: 23;  T = 50: 15: none, 20: 10, 25: 18, 30: 24, 35: 28, 40: 28, 45: 36, 50: 36, so
    the anchor is 5 - 13 frames behind.  (After 13 .. 17 frames of the T = 50 utterance the brute-force traces of its 12
    live cells still begin in two different words at column 0 and share no cell at all; from 18 frames on they meet.)"""
    seen = 0
    for T, ticks in g14_ticks(5):
        if T in (29, 50):
            seen += 1
            assert sum(t - 1 >= 15 for t, _ in ticks) >= 3
            for t, a in ticks:
                if t - 1 >= 15:                                           # the newest column is frame 15 or later
                    assert a is not None and (t - 1) - a <= 13, (T, t, a)
    assert seen == 4


# ----------------------------------------------------------------------------------------------------------------------
class FakeSettleSession:
    """Test double of `_hip.OnlineSession` with commit / tail / window, on the carried recursion and its restatement."""
    calls = 0                                         # calls that reached the backend (the refusal tests watch it)

    def __init__(self, ctx, lat, n_streams, max_frames=None, window=None):
        from sr.recognition import _hip
        assert (max_frames is None) != (window is None)
        g = lat.graphs[0]
        if lat.L != 1 or np.sum(np.asarray(g["row_state"]) < 0) != 2:
            raise _hip.Unsupported("the test double takes one loop graph")
        self.lat, self.g = lat, g
        self.n_streams, self.max_frames, self.window = int(n_streams), max_frames, window
        self.n_end = len(g["end_rows"])
        self.nes = np.asarray(g["row_state"]) < 0
        self.streams = [CarriedDecode(self.nes, lat._dense(g), g["end_rows"]) for _ in range(self.n_streams)]
        self.sd = [None] * self.n_streams

    def _sd(self, k, row_label):
        if self.sd[k] is None:
            self.sd[k] = SettledDecode(self.streams[k], row_label)
        return self.sd[k]

    def push(self, batch, ids, first=None, count=None):
        type(self).calls += 1
        ids = np.asarray(ids, dtype=np.int64)
        assert len(ids) == batch.U == len(set(ids.tolist())) and ids.min() >= 0 and ids.max() < self.n_streams
        first = np.zeros(batch.U, dtype=np.int64) if first is None else np.asarray(first)
        count = batch.lengths - first if count is None else np.asarray(count)
        settled = np.array([0 if self.sd[k] is None else self.sd[k].settled_frames for k in ids])
        if self.window is not None:
            assert np.all(self.frames()[ids] + count - settled <= self.window)
        else:
            assert np.all(self.frames()[ids] + count <= self.max_frames)
        for u, k in enumerate(ids):
            E, _ = self.lat._emissions(batch, u, self.g)
            self.streams[k].push(E[:, first[u]:first[u] + count[u]])

    def reset(self, ids=None):
        for k in (range(self.n_streams) if ids is None else ids):
            self.streams[int(k)].reset()
            self.sd[int(k)] = None

    def frames(self):
        return np.array([s.t for s in self.streams], dtype=np.int64)

    def _labels(self, k, rl):
        path = self.streams[k].result()[2]
        return O.path_to_words(path, rl < 0, rl) if len(path) else []

    def result(self, ids=None, row_label=None, max_labels=None, want_path=False):
        assert self.window is None and not want_path
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        out = self.tail(ids)
        if row_label is not None:
            rl = np.asarray(row_label)
            out["labels"] = [np.array(self._labels(int(k), rl), dtype=np.int32) for k in ids]
        return out

    def commit(self, ids=None, row_label=None, max_labels=None):
        type(self).calls += 1
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        assert len(set(ids.tolist())) == len(ids)
        new = [self._sd(int(k), np.asarray(row_label)).commit() for k in ids]
        return dict(settled_frames=np.array([self.sd[int(k)].settled_frames for k in ids], dtype=np.int64),
                    labels=[np.array(w, dtype=np.int32) for w in new])

    def tail(self, ids=None, row_label=None, max_labels=None):
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        res = [self.streams[int(k)].result() for k in ids]
        out = dict(end_cost=np.array([r[0] for r in res]).reshape(len(ids), self.n_end),
                   best_end=np.array([r[1] for r in res], dtype=np.int32), frames=self.frames()[ids])
        if row_label is not None:
            rl = np.asarray(row_label)
            out["labels"] = []
            for k in ids:
                C = [] if self.sd[int(k)] is None else self.sd[int(k)].words
                L = self._labels(int(k), rl)
                assert L[:len(C)] == C
                out["labels"].append(np.array(L[len(C):], dtype=np.int32))
        return out

    def close(self):
        pass


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", FakeSettleSession, raising=False)
    monkeypatch.setattr(FakeSettleSession, "calls", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


W_, N_, M_, D_ = 4, 3, 2, 3


def make_models(rng):
    import sr.recognition as R
    means = rng.normal(size=(W_, N_, M_, D_)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W_, N_, M_, D_))
    w = rng.dirichlet(np.ones(M_), size=(W_, N_))
    hmms = []
    for i in range(W_):
        h = R.HMM(N_)
        h.gmm_states = []
        for s in range(N_):
            g = R.GMM(means[i, s, 0].copy(), vars_[i, s, 0].copy(), M_)
            g.update_models(means[i, s].copy(), vars_[i, s].copy(), w[i, s].copy())
            h.gmm_states.append(g)
        h.transitions = word_trans(rng, N_)
        hmms.append(h)

    def utterance(words):
        segs = []
        for wd in words:
            Tw = int(rng.integers(2 * N_, 3 * N_ + 3))
            st = np.minimum(np.arange(Tw) * N_ // Tw, N_ - 1)
            segs.append(means[wd, st, 0] + 0.3 * rng.normal(size=(Tw, D_)))
        return np.concatenate(segs)
    return hmms, utterance


@pytest.mark.parametrize("windowed", [False, True])
def test_commit_settled_and_window_bookkeeping(fake_backend, windowed):
    """Interleaved subsets, commits of subsets, finish / reset and reuse of an id: `settled` grows by what `commit` returns,
    is a prefix of `result` and of the final decode, and `result` is `decode_batch` of what a stream has been given -- with
    full history and with a window far shorter than the streams."""
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(21)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=0.4)
    WINDOW = 40
    utts = {k: utterance(rng.integers(0, W_, size=rng.integers(14, 18))) for k in range(5)}
    assert min(len(x) for x in utts.values()) >= 2 * WINDOW
    on = dec.online(5, window=WINDOW) if windowed else dec.online(5, max(len(x) for x in utts.values()))
    pos = {k: 0 for k in range(5)}
    words, frames = on.settled()
    assert words == [[]] * 5 and frames.tolist() == [0] * 5
    assert on.commit() == [[]] * 5 and on.result()[0] == [[]] * 5         # nothing pushed yet
    reused = False
    for tick in range(200):
        live = [k for k in range(5) if pos[k] < len(utts[k])]
        if not live:
            break
        ids = [int(k) for k in rng.permutation(live)[:rng.integers(1, len(live) + 1)]]
        lens = [int(rng.integers(0, 6)) for _ in ids]
        on.push(ids, [utts[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)])
        for k, c in zip(ids, lens):
            pos[k] = min(pos[k] + c, len(utts[k]))
        sub = ids[:max(1, len(ids) // 2)] if tick % 3 else ids            # commits of a subset: the others keep their anchor
        before, before_frames = on.settled(sub)
        new = on.commit(sub)
        after, after_frames = on.settled(sub)
        assert after == [b + n for b, n in zip(before, new)] and np.all(after_frames >= before_frames)
        assert np.all(after_frames <= np.maximum(on.frames[sub] - 1, 0))
        done = [k for k in ids if pos[k] == len(utts[k])]
        if tick % 5 == 0 or done:                                         # (the double decodes the whole prefix: not every tick)
            b = _hip.Batch(dec.ctx, [utts[k][:pos[k]] for k in ids])
            ref_words = dec.decode_batch(b)[0]
            got, info = on.result(ids)
            assert got == ref_words and info["frames"].tolist() == [pos[k] for k in ids]
            for k, ref in zip(ids, ref_words):
                C = on.settled([k])[0][0]
                assert C == ref[:len(C)]
        if done and not reused:
            k = done[0]
            assert len(on.settled([k])[0][0]) >= 3                         # words were final long before the end
            fw, fi = on.finish([k])
            assert fw == dec.decode_batch(_hip.Batch(dec.ctx, [utts[k]]))[0]
            assert on.frames[k] == 0 and on.settled([k])[0] == [[]] and on.settled([k])[1].tolist() == [0]
            utts[k], pos[k], reused = utterance([1, 2, 0, 3, 1, 2, 0, 3]), 0, True   # the id decodes a fresh utterance
    assert reused and all(pos[k] == len(utts[k]) for k in range(5))
    assert all(len(w) >= 3 for w in on.settled()[0])
    on.reset()
    assert on.frames.tolist() == [0] * 5 and on.settled()[0] == [[]] * 5 and not on.settled()[1].any()
    on.close()


def test_refusals_come_before_the_backend(fake_backend):
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(22)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop")
    for kw in (dict(), dict(max_frames=10, window=10)):                   # neither, both
        with pytest.raises(ValueError):
            dec.online(3, **kw)
    with pytest.raises(ValueError):
        dec.online(3, window=0)
    on = dec.online(3, 10)                                                # the positional form still means max_frames
    assert on.max_frames == 10 and on.window is None
    with pytest.raises(ValueError):
        on.push([0], [rng.normal(size=(11, D_))])
    on.close()
    WINDOW = 20
    on = dec.online(3, window=WINDOW)
    x = utterance([0, 1, 2, 3, 0, 1, 2, 3, 0, 1])
    on.push([2, 0], [x[:WINDOW], x[:3]])                                  # exactly the window is fine
    frames, calls = on.frames, FakeSettleSession.calls
    assert frames.tolist() == [3, 0, WINDOW]
    for ids, chunks in (([1, 2], [x[:2], x[WINDOW:WINDOW + 1]]),          # stream 2: one frame too many -- stream 1 must not move
                        ([0], [x[3:WINDOW + 1]])):                        # stream 0: 3 + 18
        with pytest.raises(ValueError, match="stream %d" % ids[-1]):
            on.push(ids, chunks)
        assert on.frames.tolist() == frames.tolist() and FakeSettleSession.calls == calls
    for bad in ([1, 1], [3], [-1]):                                       # a stream twice, ids out of range
        with pytest.raises(ValueError):
            on.commit(bad)
        assert FakeSettleSession.calls == calls
    with pytest.raises(ValueError):
        on.settled([3])
    with pytest.raises(ValueError):
        on.result([2], want_path=True)
    with pytest.raises(ValueError):
        on.finish([2], want_path=True)
    assert on.frames.tolist() == frames.tolist()                          # (the refused finish has reset nothing)
    # a commit moves the window on: the stream takes frames again, far past the window in total
    pos = WINDOW
    while pos < len(x):
        on.commit([2])
        room = WINDOW - (on.frames[2] - on.settled([2])[1][0])
        assert room > 0, "the traces of this stream meet within the window"
        on.push([2], [x[pos:pos + room]])
        pos = min(pos + room, len(x))
    assert on.frames[2] == len(x) >= 3 * WINDOW
    on.commit([2])
    C = on.settled([2])[0][0]
    assert len(C) >= 2 and on.result([2])[0][0][:len(C)] == C
    on.reset([2])                                                         # reset clears the anchor: the window is whole again
    assert on.settled([2])[0] == [[]] and on.settled([2])[1].tolist() == [0]
    on.push([2], [x[:WINDOW]])
    assert on.frames.tolist() == [3, 0, WINDOW]
    on.close()
