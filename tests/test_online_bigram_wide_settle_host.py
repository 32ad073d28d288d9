# -*- coding: utf-8 -*-
"""The settled prefix of an online decode with a BIGRAM grammar of MORE THAN 16 WORDS, on the host (no GPU).

DEFINITIONS as in tests/test_online_settle_host.py and tests/test_online_bigram_settle_host.py.  Beyond 16 words nothing in
the definitions changes; what changes is the device mapping (a wave per stream, lane = word), whose one cross-lane step is
THE HOP: in one column several live first states leave through their entry rows to DIFFERENT words, across the 16-lane
groups of the wave.

1. The row-level restatement (tests/online_settle_ref.py on tests/online_ref.py) against brute force on
   `packed_bigram_lattice` graphs of 17, 33 and 64 words, n in {2, 5, 8}, skip arcs on and off, +inf pairs and words that
   cannot start, favoured emissions, chunks of 0 to 4 frames, T = 6 n + 60.  THE INPUT CONDITIONS are asserted from the
   restatement before anything else is compared: the anchor advances at 3 ticks or more; a settled path passes an entry row;
   at least 3/4 of the ticks with >= 2 frames have a finite chosen end; at least one column in which live first states hop
   to two different words; at least one hop that crosses a 16-lane group.
2. The bit-level restatement (tests/online_bigram_wide_settle_ref.py: records in the gh_bigram_wide_hb layout, a ring of
   columns, the mask walk with the 6-bit hop) equals the row-level one at every tick -- carried column, anchor, words, new
   words, flag 0 -- with a ring short enough to wrap.
3. The host logic of `OnlineBigramDecoder` with `wide="settle"` on test doubles: routing at 17 and at 10 words, commit /
   settled / settled_times / windowed result / times, a push past the window that reaches no backend, `wide=True` that
   keeps refusing `window=` and `settle=True`, a bad `wide` value.
4. The ABI entry is in the header, in the ctypes table and in the library."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import fake_hip
from conftest import ROOT
from online_bigram_wide_settle_ref import BigramWideSettle, BigramWideSweep, HopLog, bigram_wide_hb
from online_ref import CarriedDecode
from oracle import ref_numpy as O
from test_online_bigram_host import random_chunks
from test_online_bigram_settle_host import FakeBigramSettleSession, bigram_graph
from test_online_bigram_wide_host import D_, bigram_decoder, make_models
from test_online_settle_host import brute_force_anchor


def favoured_emissions(rng, nes, rw, W, n, T):
    """The recipe of test_online_bigram_settle_host.py: emissions that favour a word sequence (without them nothing
    separates the words and nothing settles)."""
    E = np.where(nes[:, None], 0.0, rng.uniform(3.0, 9.0, size=(len(nes), T)))
    t = 0
    while t < T:
        wd, Tw = int(rng.integers(0, W)), int(rng.integers(n, 2 * n + 3))
        for k in range(min(Tw, T - t)):
            E[np.flatnonzero(rw == wd)[min(k * n // Tw, n - 1)], t + k] = rng.uniform(0.1, 0.6)
        t += Tw
    return E


def restate(nes, rw, trans, ends, W, n, E, chunks):
    """The row-level restatement fed E in `chunks` with a commit after every chunk: (the HopLog, per tick dict(frames,
    anchor, words, new, tail: unsettled frames before the commit, col: the carried column, entry: the settled path passes
    an entry row, finite: the chosen end is a live cell, labels: the words of the carried decode's own result))."""
    cd = CarriedDecode(nes, trans, ends)
    sd = HopLog(cd, rw, W, n)
    t, ticks = 0, []
    for c in chunks:
        cd.push(E[:, t:t + c])
        t += c
        tail = t - sd.settled_frames
        before = list(sd.words)
        new = sd.commit()
        assert sd.words == before + new                           # commits only ever extend
        entry = False
        if sd.anchor is not None:
            rows = sd.path_from(sd.anchor[1], sd.anchor[0])[:, 0]
            entry = bool(np.any(nes[rows] & (rows > 0)))
        ec, bi, path = cd.result()
        ticks.append(dict(frames=t, anchor=sd.anchor, words=list(sd.words), new=new, tail=tail, col=cd.col.copy(), entry=entry,
                          finite=bool(bi >= 0 and np.isfinite(ec[bi])), labels=O.path_to_words(path, nes, rw) if len(path) else []))
    assert t == E.shape[1]
    return sd, ticks


def against_brute_force(sd, ticks, nes, rw):
    """Every tick's anchor is the latest column <= T - 2 in which the traces of ALL live cells sit in one cell, its words
    are `O.path_to_words` of the path through it, and they are a prefix of the decode of this and of every later prefix
    whose chosen end is finite (the carried decode's result: bitwise the whole decode, tests/test_online_bigram_wide_host.py)."""
    cd = sd.cd
    for k, tk in enumerate(ticks):
        at = types.SimpleNamespace(t=tk["frames"], R=cd.R, is_nes=cd.is_nes, col=tk["col"], bp=cd.bp)   # the decode as it stood
        bf = brute_force_anchor(at)
        if bf is None:
            assert tk["anchor"] is None and tk["words"] == []
        else:
            assert tk["anchor"] == (bf[0], bf[1]) and bf[0] <= tk["frames"] - 2
            assert tk["words"] == O.path_to_words(bf[2], nes, rw)
        if tk["frames"] >= 2 and tk["finite"]:
            for earlier in ticks[:k + 1]:                          # this commit's words and every earlier one's
                assert earlier["words"] == tk["labels"][:len(earlier["words"])]


def assert_input_conditions(sd, ticks):
    """What the issue asks of the inputs, from the restatement alone.  Conditions, not tolerances."""
    anchors = [tk["anchor"] for tk in ticks]
    advanced = sum(a is not None and a != b for a, b in zip(anchors, [None] + anchors[:-1]))
    two = [tk for tk in ticks if tk["frames"] >= 2]
    finite = sum(tk["finite"] for tk in two)
    got = (advanced, any(tk["entry"] for tk in ticks), finite, len(two), sd.two_word_columns(), sd.crossing_hops())
    assert advanced >= 3 and got[1] and 4 * finite >= 3 * len(two) and got[4] >= 1 and got[5] >= 1, got
    return got


SHAPES = [(17, 2, False), (17, 5, True), (17, 8, False), (33, 2, False), (33, 5, False), (33, 8, True),
          (64, 2, False), (64, 5, True), (64, 8, True)]
shape_id = lambda s: "W%d-n%d-%s" % (s[0], s[1], "skip" if s[2] else "plain")


@pytest.fixture(scope="module", params=SHAPES, ids=shape_id)
def restated(request):
    """Per shape: the graph, the emissions, the chunks and the row-level restatement, with the input conditions asserted
    on it.  Computed once, shared by (1) and (2)."""
    W, n, skip = request.param
    rng = np.random.default_rng(7700 + 100 * W + 2 * n + skip)
    nes, rw, trans, ends, B, init = bigram_graph(rng, W, n, skip, rng.uniform(0.1, 0.3))
    assert np.isinf(B).any() and np.isinf(init).any()              # +inf pairs and words that cannot start
    T = 6 * n + 60
    E = favoured_emissions(rng, nes, rw, W, n, T)
    chunks = random_chunks(rng, T)
    assert 0 in chunks and 4 in chunks
    sd, ticks = restate(nes, rw, trans, ends, W, n, E, chunks)
    assert_input_conditions(sd, ticks)                             # before anything is compared
    return dict(W=W, n=n, skip=skip, nes=nes, rw=rw, trans=trans, ends=ends, E=E, chunks=chunks, sd=sd, ticks=ticks)


def test_restatement_equals_brute_force_on_wide_bigram_graphs(restated):
    against_brute_force(restated["sd"], restated["ticks"], restated["nes"], restated["rw"])


def test_bit_level_restatement_equals_the_row_level_one(restated):
    r = restated
    W, n, skip, E = r["W"], r["n"], r["skip"], r["E"]
    ring_cols = max(tk["tail"] for tk in r["ticks"]) + 1
    assert ring_cols < E.shape[1] // 2, "the ring must wrap"
    sw = BigramWideSweep(r["trans"], W, n, ring_cols=ring_cols)
    assert sw.skip == skip and sw.hb == bigram_wide_hb(n, skip) == n + 7 + (n - 2 if skip else 0) <= 32
    ws = BigramWideSettle(sw)
    t = 0
    for c, tk in zip(r["chunks"], r["ticks"]):
        sw.push(E[:, t:t + c])
        t += c
        if t:
            np.testing.assert_array_equal(sw.prev[:, :W], tk["col"][sw.row])     # the carried column, bitwise
        assert ws.commit() == tk["new"] and ws.words == tk["words"] and ws.flag == 0
        assert (None if ws.anchor is None else (ws.anchor[0], ws.row_of(ws.anchor[1], ws.anchor[2]))) == tk["anchor"]
    # the hops of the bit-level walks are the hops of the row-level ones
    got = {}
    for j, hoppers in ws.passed:
        got.setdefault(j, set()).update(hoppers)
    assert got == r["sd"].hops
    assert any(len({v for _, v in h}) >= 2 for _, h in ws.passed) and any(l // 16 != v // 16 for _, h in ws.passed for l, v in h)


# ----------------------------------------------------------------------------------------------------------------------
class Recorded(FakeBigramSettleSession):
    """The double of test_online_bigram_settle_host.py (real results from the row-level restatement) that records how it
    was constructed."""
    how = []                                          # (class, number of positional arguments, keywords) of every construction

    def __init__(self, *args, **kw):
        Recorded.how.append((type(self), len(args), dict(kw)))
        super().__init__(*args, **kw)


class FakeWide(Recorded):
    pass


class FakeNarrow(Recorded):
    pass


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineBigramSession", FakeNarrow, raising=False)
    monkeypatch.setattr(_hip, "OnlineBigramWideSession", FakeWide, raising=True)
    monkeypatch.setattr(Recorded, "how", [])
    monkeypatch.setattr(FakeBigramSettleSession, "calls", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def test_routing_of_wide_settle_at_17_and_at_10_words(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import OnlineBigramDecoder
    rng = np.random.default_rng(71)
    hmms, _ = make_models(rng, 17)
    dec = bigram_decoder(rng, hmms)
    how = Recorded.how
    on = dec.online_bigram(2, max_frames=9, wide="settle")                 # full history: the four positional arguments of before
    assert type(on) is OnlineBigramDecoder and on.wide and not on.settles and how[-1] == (FakeWide, 4, {})
    assert on.max_frames == 9 and on.window is None
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(_hip.Unsupported):
            call([0])
    on = dec.online_bigram(2, max_frames=9, settle=True, wide="settle")
    assert on.wide and on.settles and on.max_frames == 9 and on.window is None and how[-1] == (FakeWide, 4, dict(settle=True))
    on = dec.online_bigram(2, window=7, wide="settle")
    assert on.wide and on.settles and on.window == 7 and on.max_frames is None and how[-1] == (FakeWide, 3, dict(window=7))
    on = dec.online_bigram(2, window=7, settle=True, wide="settle")
    assert on.settles and how[-1] == (FakeWide, 3, dict(window=7))
    on = OnlineBigramDecoder(dec, 2, None, 7, None, None, False, False, "settle")   # the keyword is the last positional argument
    assert on.wide and how[-1] == (FakeWide, 3, dict(window=7))
    made = len(how)
    # wide=True keeps refusing, with the words the older tests match and the way to go
    for kw in (dict(window=7), dict(max_frames=9, settle=True), dict(window=7, settle=True)):
        with pytest.raises(_hip.Unsupported, match="not built yet") as e:
            dec.online_bigram(2, wide=True, **kw)
        assert 'wide="settle"' in str(e.value)
    for bad in ("yes", "Settle", 2, None, 1.0, ()):
        with pytest.raises(ValueError, match="wide"):
            dec.online_bigram(2, max_frames=9, wide=bad)
    for kw in (dict(), dict(max_frames=5, window=5), dict(window=0), dict(max_frames=0, settle=True)):
        with pytest.raises(ValueError):
            dec.online_bigram(2, wide="settle", **kw)
    assert len(how) == made                                                # refused before a session is made
    on = dec.online_bigram(2, max_frames=9, wide=True)                     # ... and serves what it served
    assert on.wide and not on.settles and how[-1] == (FakeWide, 4, {})
    # 10 words: the permission changes nothing, the narrow class is asked as ever
    hmms10, _ = make_models(rng, 10)
    dec10 = bigram_decoder(rng, hmms10)
    for wide in (False, "settle"):
        on = dec10.online_bigram(2, max_frames=9, wide=wide)
        assert not on.wide and not on.settles and how[-1] == (FakeNarrow, 4, {})
        on = dec10.online_bigram(2, max_frames=9, settle=True, wide=wide)
        assert not on.wide and on.settles and how[-1] == (FakeNarrow, 4, dict(settle=True))
        on = dec10.online_bigram(2, window=7, wide=wide)
        assert not on.wide and on.settles and how[-1] == (FakeNarrow, 3, dict(window=7))


@pytest.mark.parametrize("windowed", [False, True])
def test_wide_settle_commit_settled_result_and_times(fake_backend, windowed):
    """Interleaved pushes and commits on a 19-word bigram decoder with times=True: `settled` / `settled_times` grow by what
    `commit(want_times=True)` returns, `result` is settled + tail and equals the carried decode of the prefix (words and
    begins), `finish` frees an id and it decodes a fresh utterance -- with full history and with a window far shorter than
    the streams."""
    from sr.recognition import _hip
    from sr.recognition.batch import path_to_word_times
    rng = np.random.default_rng(72)
    W = 19
    hmms, utterance = make_models(rng, W)
    dec = bigram_decoder(rng, hmms, forbid=0.1)
    g = dec.lat.graphs[0]
    nes = np.asarray(g["row_state"]) < 0
    WINDOW = 45
    utts = {k: utterance(rng.integers(0, W, size=int(rng.integers(18, 22)))) for k in range(3)}
    assert min(len(x) for x in utts.values()) >= 2 * WINDOW
    on = dec.online_bigram(3, window=WINDOW, times=True, wide="settle") if windowed else \
        dec.online_bigram(3, max_frames=max(len(x) for x in utts.values()), settle=True, times=True, wide="settle")
    assert type(on.session) is FakeWide and on.wide and on.settles
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
    assert any(wd >= 16 for w in on.settled()[0] for wd in w)              # words beyond the first 16 settle too
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
    rng = np.random.default_rng(73)
    W = 18
    hmms, utterance = make_models(rng, W)
    dec = bigram_decoder(rng, hmms, forbid=0.1)
    WINDOW = 40
    on = dec.online_bigram(3, window=WINDOW, wide="settle")
    assert type(on.session) is FakeWide
    x = utterance(rng.integers(0, W, size=30))
    assert len(x) >= 3 * WINDOW
    on.push([2, 0], [x[:WINDOW], x[:3]])                                  # exactly the window is fine
    frames, calls = on.frames, FakeBigramSettleSession.calls
    assert frames.tolist() == [3, 0, WINDOW]
    for ids, chunks in (([1, 2], [x[:2], x[WINDOW:WINDOW + 1]]),          # stream 2: one frame too many -- stream 1 must not move
                        ([0], [x[3:WINDOW + 1]])):
        with pytest.raises(ValueError, match="stream %d" % ids[-1]):
            on.push(ids, chunks)
        assert on.frames.tolist() == frames.tolist() and FakeBigramSettleSession.calls == calls
    for bad in ([1, 1], [3], [-1]):
        with pytest.raises(ValueError):
            on.commit(bad)
        assert FakeBigramSettleSession.calls == calls
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
    assert re.search(r"\bint\s+gh_online_create_bigram_wide_settle\s*\(", text)
    assert _hip.SIGNATURES["gh_online_create_bigram_wide_settle"] == _hip.SIGNATURES["gh_online_create_wide_settle"]
    assert hasattr(ctypes.CDLL(built_library), "gh_online_create_bigram_wide_settle")
    assert list(inspect.signature(_hip.OnlineBigramWideSession.__init__).parameters)[1:] == ["ctx", "lat", "n_streams", "max_frames", "window",
                                                                                              "settle"]
