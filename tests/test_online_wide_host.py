# -*- coding: utf-8 -*-
"""Online decoding for vocabularies of more than 16 words, on the host (no GPU).

1. The carried recursion (tests/online_ref.py) on `O.loop_grammar` graphs of 17 to 20 words against the oracle's decode
   of EVERY prefix of >= 2 frames, bitwise: the reference semantics the wide session is held to do not depend on the
   word count.
2. The routing of `sr.recognition.batch.OnlineDecoder` on test doubles of the two session classes: up to 16 words go to
   `_hip.OnlineSession`, more to `_hip.OnlineWideSession`; `window=` is refused with no session made; commit / settled /
   settled_times are refused; a ValueError push reaches no backend; times=True begins come via `path_to_word_times`.
3. The ABI entry is in the header and in the ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest

import fake_hip
from conftest import ROOT
from online_ref import CarriedDecode
from oracle import ref_numpy as O
from test_online_host import random_chunks, whole, word_trans, words_of


@pytest.mark.parametrize("W", [17, 18, 19, 20])
def test_carried_recursion_equals_the_whole_decode_of_every_prefix(W):
    rng = np.random.default_rng(1700 + W)
    n = 2 + W % 3
    skip = bool(W % 2)
    nes, rw, rs, trans, ends = O.loop_grammar([word_trans(rng, n, skip) for _ in range(W)], n, float(rng.choice([0.0, 0.7])))
    R = len(nes)
    assert R == 2 + W * n and len(ends) == W
    T = 14
    E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(R, T)))
    # a few cheap words, so that paths pass through several of the 17+ words
    for k, wd in enumerate(rng.integers(0, W, size=4)):
        E[np.flatnonzero(rw == wd), 3 * k:3 * k + 4] *= 0.1
    cd = CarriedDecode(nes, trans, ends)
    t, seen_words = 0, set()
    for c in random_chunks(rng, T):
        cd.push(E[:, t:t + c])
        t += c
        if t < 2 or c == 0:
            continue
        costs_k, ec_k, bi_k, path_k = whole(E[:, :t], nes, trans, ends)
        np.testing.assert_array_equal(cd.col, costs_k[:, -1])
        ec, bi, path = cd.result()
        np.testing.assert_array_equal(ec, ec_k)
        assert bi == bi_k
        np.testing.assert_array_equal(path, path_k)
        seen_words.update(words_of(path, nes, rw))
    assert t == T and len(seen_words) >= 2


# ----------------------------------------------------------------------------------------------------------------------
class FakeLoopSession:
    """Test double of `_hip.OnlineSession` / `_hip.OnlineWideSession` on the carried recursion."""
    made = 0                                          # sessions constructed
    pushes = 0                                        # calls that reached the backend

    def __init__(self, ctx, lat, n_streams, max_frames=None, window=None):
        from sr.recognition import _hip
        FakeLoopSession.made += 1
        g = lat.graphs[0]
        if lat.L != 1 or np.sum(np.asarray(g["row_state"]) < 0) != 2 or max_frames is None:
            raise _hip.Unsupported("the test double takes one loop graph and max_frames")
        self.lat, self.g = lat, g
        self.n_streams, self.max_frames = int(n_streams), int(max_frames)
        self.n_end = len(g["end_rows"])
        nes = np.asarray(g["row_state"]) < 0
        self.streams = [CarriedDecode(nes, lat._dense(g), g["end_rows"]) for _ in range(self.n_streams)]

    def push(self, batch, ids, first=None, count=None):
        FakeLoopSession.pushes += 1
        ids = np.asarray(ids, dtype=np.int64)
        first = np.zeros(batch.U, dtype=np.int64) if first is None else np.asarray(first)
        count = batch.lengths - first if count is None else np.asarray(count)
        assert np.all(self.frames()[ids] + count <= self.max_frames)
        for u, k in enumerate(ids):
            E, _ = self.lat._emissions(batch, u, self.g)
            self.streams[k].push(E[:, first[u]:first[u] + count[u]])

    def reset(self, ids=None):
        for k in (range(self.n_streams) if ids is None else ids):
            self.streams[int(k)].reset()

    def frames(self):
        return np.array([s.t for s in self.streams], dtype=np.int64)

    def result(self, ids=None, row_label=None, max_labels=None, want_path=False, want_begin=False):
        from sr.recognition.batch import path_to_word_times
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        res = [self.streams[int(k)].result() for k in ids]
        res = [(r[0], r[1], r[2] if self.streams[int(k)].t > 1 else r[2][:0]) for k, r in zip(ids, res)]
        out = dict(end_cost=np.array([r[0] for r in res]).reshape(len(ids), self.n_end),
                   best_end=np.array([r[1] for r in res], dtype=np.int32), frames=self.frames()[ids])
        if row_label is not None:
            rl = np.asarray(row_label)
            wt = [path_to_word_times(r[2], np.where(rl < 0, -1, rl), 1) for r in res]
            out["labels"] = [np.array(w, dtype=np.int32) for w, _ in wt]
            if want_begin:
                out["begins"] = [np.array(b, dtype=np.int32) for _, b in wt]
        if want_path:
            out["paths"] = [r[2] for r in res]
        return out

    def commit(self, *a, **k):
        raise AssertionError("the decoder must refuse before the session is asked")

    tail = commit

    def close(self):
        pass


class FakeNarrowSession(FakeLoopSession):
    pass


class FakeWideSession(FakeLoopSession):
    def __init__(self, ctx, lat, n_streams, max_frames):
        super().__init__(ctx, lat, n_streams, max_frames)


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", FakeNarrowSession, raising=False)
    monkeypatch.setattr(_hip, "OnlineWideSession", FakeWideSession, raising=False)
    monkeypatch.setattr(FakeLoopSession, "made", 0)
    monkeypatch.setattr(FakeLoopSession, "pushes", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


N_, M_, D_ = 3, 2, 3


def make_models(rng, W):
    import sr.recognition as R
    means = rng.normal(size=(W, N_, M_, D_)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, N_, M_, D_))
    w = rng.dirichlet(np.ones(M_), size=(W, N_))
    hmms = []
    for i in range(W):
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
            Tw = int(rng.integers(N_, 2 * N_ + 3))
            st = np.minimum(np.arange(Tw) * N_ // Tw, N_ - 1)
            segs.append(means[wd, st, 0] + 0.5 * rng.normal(size=(Tw, D_)))
        return np.concatenate(segs)
    return hmms, utterance


@pytest.mark.parametrize("W,cls", [(4, FakeNarrowSession), (16, FakeNarrowSession), (17, FakeWideSession), (20, FakeWideSession)])
def test_online_routes_by_word_count(fake_backend, W, cls):
    from sr.recognition.batch import ContinuousDecoder, OnlineDecoder
    hmms, _ = make_models(np.random.default_rng(40 + W), W)
    on = ContinuousDecoder(hmms, grammar="loop").online(n_streams=2, max_frames=8)
    assert type(on) is OnlineDecoder and type(on.session) is cls and on.wide == (W > 16)
    assert on.max_frames == 8 and on.window is None and FakeLoopSession.made == 1


def test_wide_decoder_refuses_window_and_settling(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(41)
    hmms, utterance = make_models(rng, 17)
    dec = ContinuousDecoder(hmms, grammar="loop")
    with pytest.raises(_hip.Unsupported):
        dec.online(n_streams=2, window=10)
    assert FakeLoopSession.made == 0                                      # refused before a session is made
    for bad in (dict(n_streams=0, max_frames=10), dict(n_streams=3, max_frames=0), dict(n_streams=3), dict(n_streams=3, max_frames=5, window=5)):
        with pytest.raises(ValueError):
            dec.online(**bad)
    assert FakeLoopSession.made == 0
    on = dec.online(n_streams=3, max_frames=10, times=True)
    on.push([1], [utterance([16, 0])[:6]])
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(_hip.Unsupported):
            call([1])
        with pytest.raises(_hip.Unsupported):
            call()
    assert on.frames.tolist() == [0, 6, 0]
    # a 16-word decoder keeps its window and its settled prefix (today's route: the narrow session class is asked)
    hmms16, _ = make_models(rng, 16)
    made = FakeLoopSession.made
    with pytest.raises(_hip.Unsupported, match="test double"):
        ContinuousDecoder(hmms16, grammar="loop").online(n_streams=2, window=10)
    assert FakeLoopSession.made == made + 1


def test_wide_decoder_refuses_a_bad_push_before_the_backend_is_touched(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(42)
    hmms, _ = make_models(rng, 18)
    on = ContinuousDecoder(hmms, grammar="loop").online(n_streams=3, max_frames=10)
    x = rng.normal(size=(4, D_))
    on.push([2, 0], [x, x[:3]])
    before, calls = on.frames, FakeLoopSession.pushes
    assert before.tolist() == [3, 0, 4] and calls == 1
    for ids, chunks in (([1, 1], [x, x]), ([0, 3], [x, x]), ([-1], [x]), ([0], [rng.normal(size=(4, D_ + 1))]), ([0], [x[0]]),
                        ([1, 2], [x, rng.normal(size=(7, D_))]),          # stream 2: 4 + 7 > 10 -- stream 1 must not move either
                        ([0, 1], [x])):
        with pytest.raises(ValueError):
            on.push(ids, chunks)
        assert on.frames.tolist() == before.tolist() and FakeLoopSession.pushes == calls
    b = _hip.Batch(on.decoder.ctx, [rng.normal(size=(8, D_)), x])
    for ids, kw in (([1, 2], dict(first=[0, 2], count=[8, 3])), ([1, 2], dict(first=[-1, 0])), ([1, 2], dict(count=[8, 7])), ([2, 1], dict())):
        with pytest.raises(ValueError):
            on.push_batch(ids, b, **kw)
        assert on.frames.tolist() == before.tolist() and FakeLoopSession.pushes == calls
    with pytest.raises(ValueError):
        on.push_audio([0], [np.zeros(100, dtype=np.int16)])               # no front-end
    on.push_batch([1, 2], b, first=[2, 0], count=[6, 4])                  # exactly to capacity is fine
    assert on.frames.tolist() == [3, 6, 8]


def test_wide_decoder_results_and_word_times(fake_backend):
    """`result` of a 19-word decoder in label and in path mode: the carried decode of the prefix, its begins what
    `path_to_word_times` gives for the path; finish frees the id."""
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder, path_to_word_times, path_to_words
    rng = np.random.default_rng(43)
    W = 19
    hmms, utterance = make_models(rng, W)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=0.4)
    on = dec.online(n_streams=4, max_frames=40, times=True)
    g = dec.lat.graphs[0]
    nes = np.asarray(g["row_state"]) < 0
    utts = {3: utterance([18, 2, 17]), 0: utterance([16]), 2: utterance([5, 18])}
    pos = {k: 0 for k in utts}
    some_wide_word = False
    while any(pos[k] < len(utts[k]) for k in utts):
        ids = [k for k in utts if pos[k] < len(utts[k])]
        lens = [int(rng.integers(0, 7)) for _ in ids]
        on.push(ids, [utts[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)])
        for k, c in zip(ids, lens):
            pos[k] = min(pos[k] + c, len(utts[k]))
        ids = [k for k in ids if pos[k] > 0]
        if not ids:
            continue
        b = _hip.Batch(dec.ctx, [utts[k][:pos[k]] for k in ids])
        b.loglik(dec.gmm, fetch=False)
        words, info = on.result(ids)
        wp, ip = on.result(ids, want_path=True)
        for u, k in enumerate(ids):
            cd = CarriedDecode(nes, dec.lat._dense(g), g["end_rows"])
            cd.push(dec.lat._emissions(b, u, g)[0])
            ec, bi, path = cd.result()
            if pos[k] < 2:
                path = path[:0]
            np.testing.assert_array_equal(info["end_cost"][u], ec)
            assert info["best_end"][u] == bi == ip["best_end"][u]
            np.testing.assert_array_equal(ip["paths"][u], path)
            assert words[u] == wp[u] == path_to_words(path, dec.row_state, dec.n)
            want_b = path_to_word_times(path, dec.row_state, dec.n)[1]
            assert info["begins"][u].tolist() == want_b == ip["begins"][u].tolist()
            some_wide_word = some_wide_word or any(wd >= 16 for wd in words[u])
    assert some_wide_word
    fw, fi = on.finish([3])
    assert len(fw[0]) >= 1 and len(fi["begins"][0]) == len(fw[0]) and on.frames.tolist() == [len(utts[0]), 0, len(utts[2]), 0]
    with pytest.raises(ValueError):
        on.result([9])


def test_header_and_binding_have_the_wide_entry(built_library):
    from sr.recognition import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmmhmm.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gh_online_create_wide\s*\(", text)
    assert "gh_online_create_wide" in _hip.SIGNATURES
    assert _hip.SIGNATURES["gh_online_create_wide"] == _hip.SIGNATURES["gh_online_create"]
    assert hasattr(ctypes.CDLL(built_library), "gh_online_create_wide")
    assert issubclass(_hip.OnlineWideSession, _hip.OnlineSession)
