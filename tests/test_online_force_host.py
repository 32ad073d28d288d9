# -*- coding: utf-8 -*-
"""The forced commit of an online decode (`online(..., max_tail=M)`, gh_online_force), on the host (no GPU).

DEFINITIONS (tests/online_force_ref.py).  T frames taken, c* = T - 1 - M, A: the cell in which the trace of the chosen end
arrives in column c*.  A cell of the newest column is MARKED iff its trace arrives in A in column c* -- "passes A" is meant
as in the settle walk: the cell a trace occupies in a column is the one in which it arrives there from the column behind
it, the FIRST cell of `path_from` in that column.

1. The restatement's marked set against brute force (`path_from` of every emitting row whose trace is defined): graphs of
   1, 3 and 16 words x 2 .. 8 states, without and with skip arcs.
2. The three consequences at every tick, chunk lengths 1 .. 9 and M in {1, 4, 7}: (a) after a commit T - settled_frames
   <= M; (b) the settled words are a prefix of the result of the same tick before forcing and of every later result; (c)
   the chosen end survives, so the words of the same tick do not change.  A tick at which the chosen end is +inf (the
   first N - 2 or so columns of a stream: no word has been crossed yet) forces nothing by definition, and (a) is asserted
   at the ticks at which it is finite.
3. M >= T: nothing is pruned, the columns are bitwise those of an unforced decode.
4. Constant emissions and equal arc costs: every tie rule at once, (1) and (2) again.
5. `OnlineDecoder`'s routing on a test double: natural commit, force of the streams over the bound, second commit; words
   in order, `n_forced`, the window guarantee, every refusal; with max_tail=None `force` is never called.
6. The library exports gh_online_force and the binding declares it."""
import ctypes

import numpy as np
import pytest

import fake_hip
from online_force_ref import chosen_end, force, forced_commit
from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from oracle import ref_numpy as O


def word_trans(rng, n, skip=False):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.1, 2.0)
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.1, 2.0)
        if skip and i < n - 2:
            t[i + 2, i] = rng.uniform(0.1, 2.0)
    return t


def graph(rng, W, n, skip, penalty, const=False):
    if const:
        wt = [np.where(np.isinf(word_trans(rng, n, skip)), np.inf, 1.0)] * W
    else:
        wt = [word_trans(rng, n, skip) for _ in range(W)]
    return O.loop_grammar(wt, n, penalty)


def emissions(rng, nes, T, const=False):
    return np.where(nes[:, None], 0.0, np.ones((len(nes), T)) if const else rng.uniform(0.0, 5.0, size=(len(nes), T)))


def words_of(cd, rw):
    """The words of the running hypothesis (the result's path), [] where there is none."""
    path = cd.result()[2]
    return O.path_to_words(path, cd.is_nes, rw) if len(path) else []


def first_cell_in_column(cd, r, j, c):
    """Brute force: the first cell of the back-trace of (r, j) in column c, or None where the trace ends before."""
    i = int(r)
    while j > c:
        i, j = (int(v) for v in cd.bp[j][i])
        if i == O._NOPTR:
            return None
    return i


def check_marked_against_brute_force(cd, out):
    c_star, A = out["cell"]
    for r in range(cd.R):
        if cd.is_nes[r]:
            continue
        assert (r in out["marked"]) == (first_cell_in_column(cd, r, cd.t - 1, c_star) == A), r


SIZES = [(W, n, skip) for W in (1, 3, 16) for n in range(2, 9) for skip in (False, True) if not (skip and n == 2)]


@pytest.mark.parametrize("W,n,skip", SIZES, ids=lambda v: str(int(v)))
def test_marked_set_equals_brute_force(W, n, skip):
    rng = np.random.default_rng(100 * W + 10 * n + skip)
    nes, rw, rs, trans, ends = graph(rng, W, n, skip, float(rng.choice([0.0, 1.0, 50.0])))
    T = 3 * n + 6
    E = emissions(rng, nes, T)
    cd = CarriedDecode(nes, trans, ends)
    sd = SettledDecode(cd, rw)
    forced = 0
    for t in range(T):
        cd.push(E[:, t:t + 1])
        if t % 3 == 2:
            before = cd.col.copy()
            out = force(cd, sd, 1 + t % 5)
            if out["cell"] is None:
                np.testing.assert_array_equal(cd.col, before)
                continue
            forced += 1
            check_marked_against_brute_force(cd, out)
            live = np.isfinite(before) & ~nes
            assert out["pruned"] == sum(1 for r in np.flatnonzero(live) if r not in out["marked"])
            np.testing.assert_array_equal(cd.col, np.where(live & ~np.isin(np.arange(cd.R), sorted(out["marked"])), np.inf, before))
    assert forced >= 2


def run_consequences(nes, rw, trans, ends, E, chunk, M):
    """Feeds E in chunks with a forced commit after each; checks (a), (b), (c); returns (forced ticks, largest tail seen)."""
    cd = CarriedDecode(nes, trans, ends)
    sd = SettledDecode(cd, rw)
    T, t, forced, settled_then = E.shape[1], 0, 0, []
    while t < T:
        cd.push(E[:, t:t + chunk])
        t = min(t + chunk, T)
        finite = np.isfinite(chosen_end(cd)[1])
        before = words_of(cd, rw)
        if finite:
            for C in settled_then:                                  # (b): every earlier commit against this later result
                assert C == before[:len(C)]
        new, pruned = forced_commit(cd, sd, M)
        forced += pruned > 0
        if finite:
            assert words_of(cd, rw) == before                       # (c)
            assert sd.words == before[:len(sd.words)]               # (b), same tick, the result before forcing
            assert t - sd.settled_frames <= M                       # (a)
        else:
            assert pruned == 0
        settled_then.append(list(sd.words))
    return forced


@pytest.mark.parametrize("M", [1, 4, 7])
@pytest.mark.parametrize("chunk", range(1, 10))
def test_three_consequences_at_every_tick(chunk, M):
    forced = 0
    for k, (W, n, skip, pen) in enumerate([(3, 2, False, 50.0), (5, 5, True, 50.0), (4, 3, True, 0.0), (16, 3, False, 50.0)]):
        rng = np.random.default_rng(7000 + 100 * chunk + 10 * M + k)
        nes, rw, rs, trans, ends = graph(rng, W, n, skip, pen)
        forced += run_consequences(nes, rw, trans, ends, emissions(rng, nes, 40), chunk, M)
    assert forced >= 4                                              # not vacuous: cells were pruned


def test_a_bound_no_smaller_than_the_stream_prunes_nothing():
    rng = np.random.default_rng(5)
    nes, rw, rs, trans, ends = graph(rng, 5, 4, True, 50.0)
    E = emissions(rng, nes, 30)
    plain = CarriedDecode(nes, trans, ends)
    cd = CarriedDecode(nes, trans, ends)
    sd = SettledDecode(cd, rw)
    for t in range(0, 30, 3):
        want = plain.push(E[:, t:t + 3])
        got = cd.push(E[:, t:t + 3])
        for M in (cd.t, cd.t + 1, 1000):
            assert force(cd, sd, M) == dict(pruned=0, cell=None, marked=None)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(cd.col, plain.col)
    assert sd.anchor is None                                        # (nothing was committed: the tail is the stream)


@pytest.mark.parametrize("W,n,skip", [(1, 2, False), (3, 3, True), (16, 4, False), (4, 8, True)])
def test_constant_emissions_every_tie_at_once(W, n, skip):
    rng = np.random.default_rng(W + n)
    nes, rw, rs, trans, ends = graph(rng, W, n, skip, 1.0, const=True)
    E = emissions(rng, nes, 3 * n + 8, const=True)
    cd = CarriedDecode(nes, trans, ends)
    sd = SettledDecode(cd, rw)
    seen = 0
    for t in range(E.shape[1]):
        cd.push(E[:, t:t + 1])
        if t >= n and t % 2 == 0:
            out = force(cd, sd, 2)                                  # (never committed: no old anchor stands in the way)
            if out["cell"] is not None:
                check_marked_against_brute_force(cd, out)
                seen += 1
    assert seen >= 2
    force(cd, sd, 2)
    sd.commit()
    assert cd.t - sd.settled_frames <= 2
    for chunk in (1, 4):
        run_consequences(nes, rw, trans, ends, E, chunk, 3)


# ----------------------------------------------------------------------------------------------------------------------
from test_online_settle_host import FakeSettleSession, make_models, D_, W_     # noqa: E402  (the settle double, extended)


class FakeForceSession(FakeSettleSession):
    """The double of `_hip.OnlineSession` with `force`, on the restatement."""
    forces = 0

    def force(self, ids=None, max_tail=1):
        type(self).forces += 1
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        assert len(set(ids.tolist())) == len(ids) and max_tail >= 1
        out = []
        for k in ids:
            assert self.sd[int(k)] is not None, "force comes after a commit"
            out.append(force(self.streams[int(k)], self.sd[int(k)], max_tail)["pruned"])
        return np.array(out, dtype=np.int32)


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", FakeForceSession, raising=False)
    monkeypatch.setattr(FakeSettleSession, "calls", 0)
    monkeypatch.setattr(FakeForceSession, "forces", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def test_decoder_routes_commit_force_commit(fake_backend):
    """A stuck model (word_penalty = 50) through a window of 24 with max_tail = 9: pushes of up to 15 frames with a commit
    after each are never refused, the tail is bounded after every commit, the words are the restatement's per stream, and
    `n_forced` counts the commits that pruned."""
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(31)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=50.0)
    WINDOW, M = 24, 9
    utts = [utterance(rng.integers(0, W_, size=12)) for _ in range(3)]
    on = dec.online(3, window=WINDOW, max_tail=M)
    assert on.max_tail == M and on.n_forced.dtype == np.int64 and on.n_forced.tolist() == [0, 0, 0]
    # the same streams by hand: the double's own streams are the restatement, so the decoder's words must equal theirs
    pos, all_new = [0, 0, 0], [[], [], []]
    sess = on.session
    while any(pos[k] < len(utts[k]) for k in range(3)):
        ids = [k for k in range(3) if pos[k] < len(utts[k])]
        lens = [int(rng.integers(0, WINDOW - M + 1)) for _ in ids]
        on.push(ids, [utts[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)])      # never refused
        for k, c in zip(ids, lens):
            pos[k] = min(pos[k] + c, len(utts[k]))
        before = on.result(ids)[0]
        n_before = on.n_forced.copy()
        new = on.commit(ids)
        words, frames = on.settled(ids)
        after = on.result(ids)[0]
        for i, k in enumerate(ids):
            all_new[k] += new[i]
            assert words[i] == all_new[k] == sess.sd[k].words
            assert frames[i] == sess.sd[k].settled_frames
            if np.isfinite(chosen_end(sess.streams[k])[1]):
                assert on.frames[k] - frames[i] <= M
                assert after[i] == before[i] and words[i] == before[i][:len(words[i])]
            assert on.n_forced[k] - n_before[k] in (0, 1)
    assert on.n_forced.sum() >= 3 and FakeForceSession.forces >= 3
    assert min(len(u) for u in utts) >= 3 * WINDOW
    on.finish([1])
    assert on.n_forced[1] == 0 and on.n_forced[0] > 0
    on.reset()
    assert on.n_forced.tolist() == [0, 0, 0]
    on.close()


def test_without_max_tail_the_stuck_stream_wedges_and_force_is_never_called(fake_backend):
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(31)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=50.0)
    x = utterance(rng.integers(0, W_, size=12))
    on = dec.online(1, window=24)
    assert on.max_tail is None
    with pytest.raises(ValueError, match="window"):
        for t in range(0, len(x), 8):
            on.push([0], [x[t:t + 8]])
            on.commit([0])
    assert FakeForceSession.forces == 0 and on.n_forced.tolist() == [0]
    on.close()


def test_times_come_back_in_order(fake_backend, monkeypatch):
    """With times=True the begins of both commits are appended like the words (the double reports a begin per word: the
    count of words settled before it)."""
    from sr.recognition.batch import ContinuousDecoder

    def commit(self, ids=None, row_label=None, max_labels=None, want_begin=False):
        r = FakeSettleSession.commit(self, ids, row_label, max_labels)
        if want_begin:
            r["begins"] = [np.arange(len(self.sd[int(k)].words) - len(l), len(self.sd[int(k)].words), dtype=np.int32)
                           for k, l in zip(ids, r["labels"])]
        return r
    monkeypatch.setattr(FakeForceSession, "commit", commit)
    rng = np.random.default_rng(32)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=50.0)
    x = utterance(rng.integers(0, W_, size=10))
    on = dec.online(2, window=30, max_tail=6, times=True)
    for t in range(0, len(x), 10):
        on.push([1], [x[t:t + 10]])
        new, begins = on.commit([1], want_times=True)
        assert [len(b) for b in begins] == [len(w) for w in new]
    words = on.settled([1])[0][0]
    assert len(words) >= 3 and on.settled_times([1])[0] == list(range(len(words))) and on.n_forced[1] >= 1
    on.close()


def test_refusals(fake_backend, monkeypatch):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(33)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop")
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_tail"):
            dec.online(2, window=20, max_tail=bad)
        with pytest.raises(ValueError, match="max_tail"):
            dec.online(2, max_frames=20, max_tail=bad)
    for bad in (20, 21):
        with pytest.raises(ValueError, match="max_tail"):
            dec.online(2, window=20, max_tail=bad)
    on = dec.online(2, window=20, max_tail=19)
    on.close()
    on = dec.online(2, max_frames=20, max_tail=50)                        # full history: any bound
    on.close()
    assert FakeSettleSession.calls == 0 and FakeForceSession.forces == 0
    # more than 16 words: refused before the backend is touched, also where the wide session would settle
    many = [hmms[k % W_] for k in range(17)]
    wide = ContinuousDecoder(many, grammar="loop")
    made = []
    monkeypatch.setattr(_hip, "OnlineWideSession", lambda *a, **k: made.append(a), raising=False)
    for kw in (dict(max_frames=50), dict(max_frames=50, settle=True), dict(window=50, settle=True)):
        with pytest.raises(_hip.Unsupported, match="max_tail"):
            wide.online(2, max_tail=5, **kw)
    assert made == []
    # the other two grammars do not get the keyword
    big = ContinuousDecoder(hmms, grammar="bigram", bigram=rng.uniform(0.5, 2.0, size=(W_, W_)))
    with pytest.raises(TypeError):
        big.online_bigram(2, window=20, max_tail=5)
    lay = ContinuousDecoder(hmms, n_layers=2)
    with pytest.raises(TypeError):
        lay.online_layers(2, 20, max_tail=5)
    with pytest.raises(_hip.Unsupported):
        lay.online(2, window=20, max_tail=5)                              # (not the loop grammar: as without max_tail)


def test_the_library_exports_gh_online_force(built_library):
    from sr.recognition import _hip
    assert "gh_online_force" in _hip.SIGNATURES
    lib = ctypes.CDLL(built_library)
    assert lib.gh_online_force is not None
    restype, argtypes = _hip.SIGNATURES["gh_online_force"]
    assert restype is ctypes.c_int and len(argtypes) == 6
