# -*- coding: utf-8 -*-
"""The settled prefix of an online decode with a BIGRAM grammar, on the host (no GPU).

DEFINITIONS as in tests/test_online_settle_host.py.  In a bigram graph every word has its own entry row, so a path can hold
three cells of one column too: a first state, ITS word's entry row, the last state of the word that fed that row -- and
two first states of one column may leave through two different words.

1. The restatement (tests/online_settle_ref.py walks `CarriedDecode.bp`, so it is form-independent) against brute force on
   `packed_bigram_lattice` graphs decoded by the oracle -- random B with +inf pairs, +inf start costs, W in {1, 3, 16},
   n in {2, 3, 5} with and without skip arcs: at every tick the anchor is the latest column <= T - 2 in which the traces
   of ALL live cells sit in one cell; C is `O.path_to_words` of the path through it; C is a prefix of `O.decode_states` of
   this and of every later prefix whose chosen end is finite (>= 2 frames: on these graphs the oracle's walk does not
   terminate on a one-frame prefix, tests/test_online_bigram_host.py).
2. G20, the reference's own decodes of the bigram graph, in chunks of 1, 7 and 50.
3. The host logic of the OPT-IN `OnlineBigramDecoder` (`window=`, `max_frames=..., settle=True`) on a double of
   `_hip.OnlineBigramSession` that computes real results: `_room` with a window, `result` = settled + tail, `commit`
   with and without times, reset, and argument errors before any push.  The default decoder is pinned by
   tests/test_online_bigram_host.py and stays as it is.
4. The library exports gh_online_create_bigram_settle."""
import ctypes

import numpy as np
import pytest

import fake_hip
from conftest import load_golden
from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from oracle import ref_numpy as O
from test_online_bigram_host import FakeOnlineBigramSession, D_, W_, bigram_decoder, dense_of, random_costs, whole, word_trans
from test_online_settle_host import brute_force_anchor, make_models, random_chunks      # (its utterances: clean, longer words)


def run_contract(E, nes, rw, trans, ends, chunks):
    """Feeds E in `chunks`, commits after every chunk and checks the whole contract; returns per tick (frames, anchor
    column or None, a settled path passes an entry row, the chosen end is finite)."""
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
        entry = False
        if bf is None:
            assert sd.anchor is None and sd.words == []
        else:
            assert sd.anchor == (bf[0], bf[1]) and bf[0] <= t - 2
            assert sd.words == O.path_to_words(bf[2], nes, rw)
            entry = bool(np.any(nes[bf[2][:, 0]] & (bf[2][:, 0] > 0)))
        settled.append(list(sd.words))
        finite = False
        if t >= 2:
            ec, path = whole(E[:, :t], nes, trans, ends)
            finite = bool(np.isfinite(ec).any())
            if finite:
                L = O.path_to_words(path, nes, rw)
                for C in settled:                                  # this commit's C and every earlier one
                    assert C == L[:len(C)]
        ticks.append((t, None if sd.anchor is None else sd.anchor[0], entry, finite))
    assert t == E.shape[1]
    return ticks


def bigram_graph(rng, W, n, skip, forbid):
    from sr.recognition.continuous_speech import packed_bigram_lattice
    B, init = random_costs(rng, W, forbid)
    while W > 1 and not (np.isinf(B).any() and np.isinf(init).any()):     # forbidden pairs and words that cannot start
        B, init = random_costs(rng, W, forbid)
    graph, _ = packed_bigram_lattice([word_trans(rng, n, skip) for _ in range(W)], n, B, init)
    nes = graph["row_state"] < 0
    rw = np.where(nes, -1, graph["row_state"] // n)
    return nes, rw, dense_of(graph), [int(e) for e in graph["end_rows"]], B, init


SHAPES = [(W, n, skip) for W in (1, 3, 16) for n in (2, 3, 5) for skip in ((False, True) if n > 2 else (False,))]


@pytest.mark.parametrize("W,n,skip", SHAPES)
def test_restatement_equals_brute_force_on_bigram_graphs(W, n, skip):
    rng = np.random.default_rng(7100 + 100 * W + 2 * n + skip)
    advanced = entries = finite = ticks_2 = 0
    for rep in range(3):
        nes, rw, trans, ends, B, init = bigram_graph(rng, W, n, skip, rng.uniform(0.1, 0.3))
        assert W == 1 or (np.isinf(B).any() and np.isinf(init).any())
        R = len(nes)
        T = (n + 1, 3 * n + 8, 6 * n + 22)[rep]
        # emissions that favour a word sequence: without them nothing separates the words and nothing settles
        E = np.where(nes[:, None], 0.0, rng.uniform(3.0, 9.0, size=(R, T)))
        t = 0
        while t < T:
            wd, Tw = int(rng.integers(0, W)), int(rng.integers(n, 2 * n + 3))
            for k in range(min(Tw, T - t)):
                E[np.flatnonzero(rw == wd)[min(k * n // Tw, n - 1)], t + k] = rng.uniform(0.1, 0.6)
            t += Tw
        if rep == 1:
            E[rng.integers(1, R), rng.integers(0, T)] = np.inf           # an emission that underflowed
        ticks = run_contract(E, nes, rw, trans, ends, random_chunks(rng, T))
        anchors = [a for _, a, _, _ in ticks]
        advanced += sum(a is not None and a != b for a, b in zip(anchors[1:], anchors[:-1]))
        entries += any(e for _, _, e, _ in ticks)
        finite += sum(f for tt, _, _, f in ticks if tt >= 2)
        ticks_2 += sum(tt >= 2 for tt, _, _, _ in ticks)
    # not vacuous: anchors advance, settled paths pass entry rows, most prefixes have a live end
    assert advanced >= 3 and entries >= 1 and 4 * finite >= 3 * ticks_2, (advanced, entries, finite, ticks_2)


@pytest.mark.parametrize("chunk", [1, 7, 50])
def test_G20_in_chunks(chunk):
    """The contract on the reference's own bigram decodes (random, forbidden and tied costs); the final settled words are
    a prefix of the golden digits and, fed 7 frames at a time, some utterance settles a word before its audio ends."""
    g = load_golden("G20_bigram_grammar")
    early = 0
    for case in range(int(g["n_cases"])):
        pp = "c%d_" % case
        means, vars_, w = g[pp + "means"], g[pp + "vars"], g[pp + "w"]
        rw, rs, ends = g[pp + "row_word"], g[pp + "row_state"], g[pp + "ends"]
        R = len(rw)
        nes = rw < 0
        trans = np.full((R, R), np.inf)
        trans[g[pp + "arc_to"], g[pp + "arc_from"]] = g[pp + "arc_cost"]
        states = [None if nes[r] else (means[rw[r], rs[r]], vars_[rw[r], rs[r]], w[rw[r], rs[r]]) for r in range(R)]
        for u in range(int(g["n_utts"])):
            E = O.emission_matrix(g[pp + "x%d" % u], states)
            T = E.shape[1]
            ticks = run_contract(E, nes, rw, trans, [int(e) for e in ends], [min(chunk, T - t) for t in range(0, T, chunk)])
            cd = CarriedDecode(nes, trans, ends)
            sd = SettledDecode(cd, rw)
            cd.push(E)
            sd.commit()
            digits = list(g[pp + "digits%d" % u])
            assert sd.words == digits[:len(sd.words)]
            early += any(a is not None for tt, a, _, _ in ticks if tt < T)
    assert chunk == 50 or early >= 1


# ----------------------------------------------------------------------------------------------------------------------
class FakeBigramSettleSession(FakeOnlineBigramSession):
    """Test double of the opt-in `_hip.OnlineBigramSession`: the parent double's carried recursion, plus commit / tail on
    its restatement and the window check of a push.  Made without settle= or window= it is the parent double."""
    calls = 0                                         # calls that reached the backend (the refusal tests watch it)

    def __init__(self, ctx, lat, n_streams, max_frames=None, window=None, settle=False):
        assert (max_frames is None) != (window is None)
        super().__init__(ctx, lat, n_streams, 1 << 40 if max_frames is None else max_frames)
        self.window = window                          # (a windowed double has no capacity: the parent's check never fires)
        self.settles = bool(settle) or window is not None
        self.sd = [None] * self.n_streams
        self.n_settled = [0] * self.n_streams

    def _sd(self, k, rl):
        if self.sd[k] is None:
            self.sd[k] = SettledDecode(self.streams[k], rl)
        return self.sd[k]

    def push(self, batch, ids, first=None, count=None):
        type(self).calls += 1
        if self.window is not None:
            idx = np.asarray(ids, dtype=np.int64)
            f = np.zeros(batch.U, dtype=np.int64) if first is None else np.asarray(first)
            c = batch.lengths - f if count is None else np.asarray(count)
            settled = np.array([0 if self.sd[k] is None else self.sd[k].settled_frames for k in idx])
            assert np.all(self.frames()[idx] + c - settled <= self.window)
        FakeOnlineBigramSession.push(self, batch, ids, first, count)

    def reset(self, ids=None):
        super().reset(ids)
        for k in (range(self.n_streams) if ids is None else ids):
            self.sd[int(k)], self.n_settled[int(k)] = None, 0

    def result(self, ids=None, row_label=None, max_labels=None, want_path=False, want_begin=False):
        from sr.recognition import _hip
        if self.window is not None:
            raise _hip.Unsupported("a session with a window: tail()")
        return super().result(ids, row_label, max_labels, want_path, want_begin)

    def _timed(self, path, rl):
        from sr.recognition.batch import path_to_word_times
        return path_to_word_times(path, np.where(rl < 0, -1, rl), 1)

    def commit(self, ids=None, row_label=None, max_labels=None, want_begin=False):
        from sr.recognition import _hip
        if not self.settles:
            raise _hip.Unsupported("a bigram session has no settled prefix")
        type(self).calls += 1
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        assert len(set(ids.tolist())) == len(ids)
        rl = np.asarray(row_label)
        labels, begins = [], []
        for k in (int(v) for v in ids):
            sd = self._sd(k, rl)
            new = sd.commit()
            wds, bgs = self._timed(sd.path_from(sd.anchor[1], sd.anchor[0]), rl) if sd.anchor is not None else ([], [])
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
            raise _hip.Unsupported("a bigram session has no settled prefix")
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        out = FakeOnlineBigramSession.result(self, ids, row_label, max_labels, False, want_begin)
        if row_label is not None:
            for i, k in enumerate(int(v) for v in ids):
                C = [] if self.sd[k] is None else self.sd[k].words
                assert out["labels"][i].tolist()[:len(C)] == C
                out["labels"][i] = out["labels"][i][len(C):]
                if want_begin:
                    out["begins"][i] = out["begins"][i][len(C):]
        return out


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineBigramSession", FakeBigramSettleSession, raising=False)
    monkeypatch.setattr(FakeBigramSettleSession, "calls", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def long_utterance(rng, utterance, n_words):
    return utterance(rng.integers(0, W_, size=n_words))


@pytest.mark.parametrize("windowed", [False, True])
def test_opt_in_decoder_commit_settled_result_and_times(fake_backend, windowed):
    """Interleaved subsets, commits of subsets, finish / reset and reuse of an id, with times=True: `settled` /
    `settled_times` grow by what `commit(want_times=True)` returns, `result` is settled + tail and equals `decode_batch`
    (words and begins) of what a stream has been given -- with full history and with a window far shorter than the
    streams."""
    from sr.recognition import _hip
    from sr.recognition.batch import OnlineBigramDecoder, OnlineDecoder, path_to_word_times
    rng = np.random.default_rng(31)
    hmms, utterance = make_models(rng)
    dec = bigram_decoder(rng, hmms)
    g = dec.lat.graphs[0]
    nes = np.asarray(g["row_state"]) < 0
    WINDOW = 45
    utts = {k: long_utterance(rng, utterance, int(rng.integers(12, 15))) for k in range(4)}
    assert min(len(x) for x in utts.values()) >= 2 * WINDOW
    if windowed:
        on = dec.online_bigram(4, window=WINDOW, times=True)
        assert on.window == WINDOW and on.max_frames is None
    else:
        on = dec.online_bigram(4, max_frames=max(len(x) for x in utts.values()), settle=True, times=True)
        assert on.window is None
    assert isinstance(on, OnlineBigramDecoder) and isinstance(on, OnlineDecoder) and on.settles
    pos = {k: 0 for k in range(4)}
    assert on.settled()[0] == [[]] * 4 and on.commit() == [[]] * 4 and on.result()[0] == [[]] * 4
    reused = False
    for tick in range(300):
        live = [k for k in range(4) if pos[k] < len(utts[k])]
        if not live:
            break
        ids = [int(k) for k in rng.permutation(live)[:rng.integers(1, len(live) + 1)]]
        lens = [int(rng.integers(0, 6)) for _ in ids]
        on.push(ids, [utts[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)])
        for k, c in zip(ids, lens):
            pos[k] = min(pos[k] + c, len(utts[k]))
        sub = ids[:max(1, len(ids) // 2)] if tick % 3 else ids            # commits of a subset: the others keep their anchor
        (before, before_frames), before_t = on.settled(sub), on.settled_times(sub)
        if tick % 2:
            new, new_t = on.commit(sub, want_times=True)
        else:
            new, new_t = on.commit(sub), None
        (after, after_frames), after_t = on.settled(sub), on.settled_times(sub)
        assert after == [b + n for b, n in zip(before, new)] and np.all(after_frames >= before_frames)
        assert np.all(after_frames <= np.maximum(on.frames[sub] - 1, 0))
        assert [len(a) for a in after_t] == [len(a) for a in after]
        if new_t is not None:
            assert after_t == [b + n for b, n in zip(before_t, new_t)]
        done = [k for k in ids if pos[k] == len(utts[k])]
        if tick % 12 == 0 or done:                                         # (the double decodes the whole prefix: not every tick)
            some = [k for k in ids if pos[k] >= 2]
            if some:
                b = _hip.Batch(dec.ctx, [utts[k][:pos[k]] for k in some])
                b.loglik(dec.gmm, fetch=False)
                assert on.result(some)[0] == dec.decode_batch(b)[0]
                got, info = on.result(some)
                assert info["frames"].tolist() == [pos[k] for k in some]
                for u, k in enumerate(some):                              # words and begins: the carried decode of the prefix
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
            utts[k], pos[k], reused = utterance([1, 2, 0, 3, 1, 2, 0, 3]), 0, True   # the id decodes a fresh utterance
    assert reused and all(pos[k] == len(utts[k]) for k in range(4))
    assert all(len(w) >= 3 for w in on.settled()[0])
    if windowed:
        assert max(len(x) for x in utts.values()) > 2 * WINDOW            # streams ran far past the window
        with pytest.raises(ValueError):
            on.result([0], want_path=True)
    on.reset()
    assert on.frames.tolist() == [0] * 4 and on.settled()[0] == [[]] * 4 and not on.settled()[1].any()
    assert on.settled_times() == [[]] * 4
    on.close()


def test_opt_in_refusals_come_before_the_backend(fake_backend):
    from sr.recognition import _hip
    rng = np.random.default_rng(32)
    hmms, utterance = make_models(rng)
    dec = bigram_decoder(rng, hmms)
    for kw in (dict(), dict(max_frames=10, window=10), dict(settle=True), dict(window=0), dict(max_frames=0, settle=True)):
        with pytest.raises(ValueError):
            dec.online_bigram(3, **kw)
    with pytest.raises(ValueError):
        dec.online_bigram(0, window=10)
    assert FakeBigramSettleSession.calls == 0
    # the default object is today's: nothing settles, whatever the session could do
    on = dec.online_bigram(3, 10)
    assert on.max_frames == 10 and on.window is None and not on.settles
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(_hip.Unsupported):
            call([0])
    on.close()
    # a decoder without times refuses want_times and settled_times like OnlineDecoder
    on = dec.online_bigram(3, max_frames=10, settle=True)
    with pytest.raises(ValueError):
        on.commit([0], want_times=True)
    with pytest.raises(ValueError):
        on.settled_times([0])
    with pytest.raises(ValueError):
        on.push([0], [rng.normal(size=(11, D_))])                         # max_frames stays a hard capacity
    on.close()
    WINDOW = 40
    on = dec.online_bigram(3, window=WINDOW)
    x = long_utterance(rng, utterance, 24)
    on.push([2, 0], [x[:WINDOW], x[:3]])                                  # exactly the window is fine
    frames, calls = on.frames, FakeBigramSettleSession.calls
    assert frames.tolist() == [3, 0, WINDOW]
    for ids, chunks in (([1, 2], [x[:2], x[WINDOW:WINDOW + 1]]),          # stream 2: one frame too many -- stream 1 must not move
                        ([0], [x[3:WINDOW + 1]])):                        # stream 0: 3 + 38
        with pytest.raises(ValueError, match="stream %d" % ids[-1]):
            on.push(ids, chunks)
        assert on.frames.tolist() == frames.tolist() and FakeBigramSettleSession.calls == calls
    for bad in ([1, 1], [3], [-1]):                                       # a stream twice, ids out of range
        with pytest.raises(ValueError):
            on.commit(bad)
        assert FakeBigramSettleSession.calls == calls
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


def test_library_exports_the_settle_entry(built_library):
    import inspect
    from sr.recognition import _hip
    lib = ctypes.CDLL(built_library)
    assert hasattr(lib, "gh_online_create_bigram_settle")
    assert "gh_online_create_bigram_settle" in _hip.SIGNATURES
    assert list(inspect.signature(_hip.OnlineBigramSession.__init__).parameters)[1:] == ["ctx", "lat", "n_streams", "max_frames", "window",
                                                                                          "settle"]
