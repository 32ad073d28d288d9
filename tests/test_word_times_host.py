# -*- coding: utf-8 -*-
"""Word begin times on the host (no GPU).

THE RULE.  Take the path as decode_hmm_states returns it (end -> start, without the end cell) and walk it start -> end as
main.py:59-67 does: a word is a maximal run of cells on emitting rows between non-emitting rows, its label is the label of
the run's first cell, and its BEGIN is the column of that first cell.  Ends are not stored: word k ends where word k + 1
begins, the last one at the utterance's frame count (`word_spans`).

1. `path_to_word_times` against a restatement written here -- the loop of main.py:39-67 carrying the column -- on the
   reference's own paths in G4 (K1..K3), G14 and G20: the words are the goldens' digits, the begins the restatement's,
   strictly increasing from column 0 and below the frame count; three of them spelled out.
2. The same on the oracle's decodes of random loop, bigram and layer graphs, utterances of 0, 1 and 2 frames included.
3. `word_spans` tiles [begins[0], frames).
4. The host logic of `OnlineDecoder(times=...)` on a double of the session defined here."""
import warnings

import numpy as np
import pytest

import audio_capture_ref as A
import fake_hip
import stream_endpoints_ref as S
from conftest import load_golden
from oracle import ref_numpy as O
from stream_frontend_ref import FakeStreamFrontend
from test_online_settle_host import FakeSettleSession, make_models


def restate_word_times(path, is_nes, row_word):
    """main.py:59-67 with split_result (:39-52), every element carrying its column: reverse the path, drop consecutive
    duplicates of a row (the first cell of the row's run stays, with its column), split at the non-emitting rows keeping the
    first element of every piece."""
    cells = [(int(r), int(c)) for r, c in np.asarray(path).reshape(-1, 2)[::-1]]
    matched = [cell for i, cell in enumerate(cells) if i == 0 or cell[0] != cells[i - 1][0]]
    out, ret, found = [], None, False
    for e in matched:
        if not is_nes[e[0]]:
            if not found:
                ret, found = e, True
        elif ret is not None:
            out.append(ret)
            ret, found = None, False
    if ret is not None:
        out.append(ret)
    return [int(row_word[r]) for r, _ in out], [c for _, c in out]


def golden_paths():
    """(name, path, row_word, digits, frames) of every reference path the rule is checked on."""
    g = load_golden("G4_lattice_decode")
    for K in (1, 2, 3):
        p = "K%d_" % K
        yield "G4 " + p + "path", g[p + "path"], g[p + "row_word"], g[p + "digits"], len(g[p + "x"])
    for name, pre, n_cases in (("G14_loop_grammar", "p", 2), ("G20_bigram_grammar", "c", 3)):
        g = load_golden(name)
        for c in range(n_cases):
            pp = "%s%d_" % (pre, c)
            for u in range(int(g["n_utts"])):
                yield "%s %spath%d" % (name[:3], pp, u), g[pp + "path%d" % u], g[pp + "row_word"], g[pp + "digits%d" % u], len(g[pp + "x%d" % u])


LITERALS = {"G14 p0_path2": ([2, 3, 1, 1, 3], [0, 11, 19, 29, 40]),
            "G20 c1_path2": (None, [0, 8, 13, 25, 36]),
            "G4 K3_path": (None, [0, 17, 36])}


def test_rule_on_the_reference_paths():
    from sr.recognition.batch import path_to_word_times
    seen = set()
    for name, path, rw, digits, frames in golden_paths():
        row_state = np.where(rw < 0, -1, rw)                             # one "state" per word: label = state // 1
        words, begins = path_to_word_times(path, row_state, 1)
        assert words == [int(d) for d in digits], name
        assert (words, begins) == restate_word_times(path, rw < 0, rw), name
        assert all(isinstance(b, int) for b in begins)
        if len(begins):
            assert begins[0] == 0 and np.all(np.diff(begins) > 0) and begins[-1] < frames, name
        if name in LITERALS:
            lw, lb = LITERALS[name]
            assert begins == lb and (lw is None or words == lw), name
            seen.add(name)
    assert seen == set(LITERALS)


def random_graph(rng, kind, W, n, skip):
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    from test_online_settle_host import word_trans
    wt = [word_trans(rng, n, skip) for _ in range(W)]
    if kind == "loop":
        return packed_loop_lattice(wt, n, float(rng.choice([0.0, 0.8])))[0]
    if kind == "bigram":
        B = rng.uniform(0.0, 4.0, size=(W, W))
        B[0, W - 1] = np.inf                                             # a forbidden pair
        return packed_bigram_lattice(wt, n, B, None)[0]
    return packed_lattice(wt, n, [list(range(W))] * 3)[0]


@pytest.mark.parametrize("kind", ["loop", "bigram", "layers"])
def test_rule_on_random_decodes(kind):
    from sr.recognition.batch import path_to_word_times, path_to_words
    rng = np.random.default_rng({"loop": 1, "bigram": 2, "layers": 3}[kind])
    with_words, short = 0, {}
    for trial in range(12):
        W, n, skip = int(rng.integers(2, 5)), int(rng.integers(2, 6)), bool(trial % 2)
        g = random_graph(rng, kind, W, n, skip)
        rs = np.asarray(g["row_state"])
        R = len(rs)
        dense = np.full((R, R), np.inf)
        dense[g["arc_to"], g["arc_from"]] = g["arc_cost"]
        nes, rw = rs < 0, np.where(rs < 0, -1, rs // n)
        for T in (0, 1, 2, int(rng.integers(3, 50)), int(rng.integers(3, 50))):
            if T == 0:
                path = np.zeros((0, 2), dtype=np.int64)
            else:
                E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(R, T)))
                try:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        costs, path = O.decode_states(E, nes, dense, end_points=[[int(e), -1] for e in g["end_rows"]])
                except RuntimeError:       # a back-trace the oracle refuses: an unreachable end, and every 1-frame utterance
                                           # of these graphs (the reference's column wrap at T == 1 does not terminate)
                    continue
                path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
            short[T] = short.get(T, 0) + 1
            words, begins = path_to_word_times(path, rs, n)
            assert (words, begins) == restate_word_times(path, nes, rw), (trial, T)
            assert words == path_to_words(path, rs, n) and len(words) == len(begins)
            if T == 0:
                assert (words, begins) == ([], [])
            if T >= 2 and len(path) and np.isfinite(costs[np.asarray(g["end_rows"]), -1]).any():
                assert begins[0] == 0 and np.all(np.diff(begins) > 0) and begins[-1] < T
                with_words += len(words) >= 2
    assert with_words >= 6 and short[0] == 12 and short.get(2, 0) >= 3


def test_word_spans_tile_the_utterance():
    from sr.recognition.batch import word_spans
    assert word_spans([], 17) == []
    assert word_spans([0], 9) == [(0, 9)]
    assert word_spans(np.array([0, 11, 19, 29, 40], dtype=np.int32), 50) == [(0, 11), (11, 19), (19, 29), (29, 40), (40, 50)]
    spans = word_spans([3, 4, 10], 12)                                   # (begins need not start at 0: an online tail)
    assert spans[0][0] == 3 and spans[-1][1] == 12 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert all(isinstance(v, int) for s in spans for v in s)


# ------------------------------------------------------------------ 4: OnlineDecoder(times=...) on a double of the session
class TimedSettleSession(FakeSettleSession):
    """`FakeSettleSession` with `want_begin`: the begins are the restatement's on the carried recursion's own path.  A call
    without `want_begin` goes to the parent's methods unchanged, whose signatures do not know the keyword."""
    timed_calls = 0

    def _timed(self, k, rl):
        path = self.streams[k].result()[2]
        return restate_word_times(path, rl < 0, rl) if len(path) else ([], [])

    def result(self, ids=None, row_label=None, max_labels=None, want_path=False, want_begin=False):
        out = super().result(ids, row_label, max_labels, want_path)
        if want_begin:
            type(self).timed_calls += 1
            ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
            out["begins"] = [np.array(self._timed(int(k), np.asarray(row_label))[1], dtype=np.int32) for k in ids]
        return out

    def commit(self, ids=None, row_label=None, max_labels=None, want_begin=False):
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        before = [0 if self.sd[int(k)] is None else len(self.sd[int(k)].words) for k in ids]
        out = super().commit(ids, row_label, max_labels)
        if want_begin:
            type(self).timed_calls += 1
            out["begins"] = []
            for k, n0, new in zip(ids, before, out["labels"]):
                L, B = self._timed(int(k), np.asarray(row_label))
                assert L[n0:n0 + len(new)] == [int(w) for w in new]
                out["begins"].append(np.array(B[n0:n0 + len(new)], dtype=np.int32))
        return out

    def tail(self, ids=None, row_label=None, max_labels=None, want_begin=False):
        out = super().tail(ids, row_label, max_labels)
        if want_begin:
            type(self).timed_calls += 1
            ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
            out["begins"] = []
            for k, tail_labels in zip(ids, out["labels"]):
                B = self._timed(int(k), np.asarray(row_label))[1]
                out["begins"].append(np.array(B[len(B) - len(tail_labels):], dtype=np.int32))
        return out


@pytest.fixture
def timed_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", TimedSettleSession, raising=False)
    monkeypatch.setattr(_hip, "StreamFrontend", FakeStreamFrontend, raising=False)
    monkeypatch.setattr(_hip, "EndpointStream", S.FakeEndpointStream, raising=False)
    monkeypatch.setattr(TimedSettleSession, "timed_calls", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


@pytest.fixture
def untimed_backend(monkeypatch, built_library):
    """The double as it was before word times: a `want_begin` keyword is a TypeError."""
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", FakeSettleSession, raising=False)
    monkeypatch.setattr(_hip, "StreamFrontend", FakeStreamFrontend, raising=False)
    monkeypatch.setattr(_hip, "EndpointStream", S.FakeEndpointStream, raising=False)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def offline_times(dec, x):
    """(words, begins, frames) of the whole-utterance decode of x: the host rule on the decode's own path."""
    from sr.recognition import _hip
    b = _hip.Batch(dec.ctx, [x])
    words, r = dec.decode_batch(b, want_path=True, want_times=True)
    return words[0], [int(v) for v in r["begins"][0]], len(x)


@pytest.mark.parametrize("windowed", [False, True])
def test_begins_accumulate_over_commits_and_result_is_settled_plus_tail(timed_backend, windowed):
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(31)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=0.4)
    utts = [utterance(rng.integers(0, 4, size=9)) for _ in range(3)]
    on = dec.online(3, window=40, times=True) if windowed else dec.online(3, max_frames=max(len(x) for x in utts), times=True)
    assert on.times and on.settled_times() == [[], [], []]
    acc_w, acc_b = [[] for _ in range(3)], [[] for _ in range(3)]
    pos = [0, 0, 0]
    plain_returns = 0
    while any(p < len(x) for p, x in zip(pos, utts)):
        ids = [k for k in range(3) if pos[k] < len(utts[k])]
        lens = [int(rng.integers(0, 7)) for _ in ids]
        on.push(ids, [utts[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)])
        for k, c in zip(ids, lens):
            pos[k] = min(pos[k] + c, len(utts[k]))
        if sum(pos) % 3 == 0:                               # plain commit(ids) returns what it returns today, and still accumulates
            new_w = on.commit(ids)
            assert isinstance(new_w, list) and all(isinstance(w, list) for w in new_w)
            new_b = [on.settled_times([k])[0][len(acc_b[k]):] for k in ids]
            plain_returns += 1
        else:
            new_w, new_b = on.commit(ids, want_times=True)
        for k, w, b in zip(ids, new_w, new_b):
            assert len(w) == len(b)
            acc_w[k] += w
            acc_b[k] += b
        assert on.settled(ids)[0] == [acc_w[k] for k in ids] and on.settled_times(ids) == [acc_b[k] for k in ids]
        words, info = on.result(ids)
        for i, k in enumerate(ids):
            ref_w, ref_b, _ = offline_times(dec, utts[k][:pos[k]]) if pos[k] else ([], [], 0)
            assert words[i] == ref_w and info["begins"][i].tolist() == ref_b and info["begins"][i].dtype == np.int32
            assert ref_w[:len(acc_w[k])] == acc_w[k] and ref_b[:len(acc_b[k])] == acc_b[k]       # settled, then the tail's
    assert plain_returns > 0 and TimedSettleSession.timed_calls > 0 and sum(len(b) for b in acc_b) >= 9
    assert windowed is False or max(max(b) for b in acc_b if b) > 40     # absolute columns, past the window
    # finish follows result and clears; reset clears
    fw, fi = on.finish([1])
    assert (fw[0], fi["begins"][0].tolist()) == offline_times(dec, utts[1])[:2]
    assert on.settled_times([1]) == [[]] and on.settled([1])[0] == [[]] and on.settled_times([0]) == [acc_b[0]]
    on.reset([0])
    assert on.settled_times() == [[], [], acc_b[2]]
    on.reset()
    assert on.settled_times() == [[], [], []]


def test_times_false_changes_nothing(untimed_backend):
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(32)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=0.4)
    x = utterance([0, 1, 2, 3, 1])
    for kw in (dict(max_frames=len(x)), dict(window=40)):
        on = dec.online(2, **kw)
        assert on.times is False
        on.push([1], [x[:30]])
        new = on.commit([1])
        assert isinstance(new, list) and isinstance(new[0], list)
        words, info = on.result([1])
        assert sorted(info) == ["best_end", "end_cost", "frames"]
        with pytest.raises(ValueError, match="times=True"):
            on.commit([1], want_times=True)
        with pytest.raises(ValueError, match="times=True"):
            on.settled_times()
        fw, fi = on.finish([1])
        assert sorted(fi) == ["best_end", "end_cost", "frames"]


@pytest.mark.parametrize("times", [False, True])
def test_push_recording_turns_frames_into_recording_samples(timed_backend, times):
    from sr.audio_capture import StreamingEndpointer
    from sr.feature import StreamingFrontend
    from sr.recognition import _hip
    from stream_frontend_ref import raw_stack
    from test_stream_frontend_host import make_decoder
    rng = np.random.default_rng(5)
    dec = make_decoder(rng)
    raw = dict(A.DEFAULT_CONFIG, **{'sample rate': 16000, 'silence threshold': 100, 'speech threshold': 50, 'start boundary': 20})
    ep = StreamingEndpointer(2, dict(raw), max_chunk=1600)
    fe = StreamingFrontend(2, max_chunk=ep.max_piece)
    on = dec.online(2, max_frames=60, frontend=fe, endpointer=ep, times=times)
    x = S.burst_signal(rng, 16000, 40, [(3000, 6000), (10000, 13000)], rate=16000)
    got = []
    for t in range(0, 16000, 1600):
        got += on.push_recording([1], [x[t:t + 1600]], [t + 1600 >= 16000])
    assert len(got) == 2
    for u in got:
        if not times:
            assert sorted(u) == ["begin", "open", "stop", "stream", "words"]
            continue
        assert sorted(u) == ["begin", "begins", "open", "stop", "stream", "word_begin", "words"]
        b = _hip.Batch(dec.ctx, [raw_stack(O.mfcc_features_signal(x[u["begin"]:u["stop"]], 16000)[1])])
        words, r = dec.decode_batch(b, want_path=True, want_times=True)
        assert u["words"] == words[0] and u["begins"] == r["begins"][0].tolist() and len(u["words"]) >= 1
        assert fe.step == 160
        assert u["word_begin"] == [u["begin"] + f * 160 for f in u["begins"]]
        assert all(u["begin"] <= s < u["stop"] for s in u["word_begin"])
