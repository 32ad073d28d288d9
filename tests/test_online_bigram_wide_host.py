# -*- coding: utf-8 -*-
"""Online decoding with a bigram grammar of more than 16 words, on the host (no GPU).

1. The carried recursion (tests/online_ref.py) on `packed_bigram_lattice` graphs of 17 to 20 words -- forbidden pairs,
   words that cannot start -- against the oracle's decode of EVERY prefix of >= 2 frames, bitwise: the reference semantics
   the wide bigram session is held to do not depend on the word count.  A ONE-frame prefix is pinned against the carried
   form's own causal column, as in test_online_bigram_host.py.
2. The routing of `sr.recognition.batch.OnlineBigramDecoder` on test doubles of the two session classes: `wide=True` at 17
   words makes a `_hip.OnlineBigramWideSession` with `max_frames`, at 10 words the narrow session as without the keyword;
   `wide=True` with `window=` or `settle=True` at 17 words is refused with no session made; commit / settled /
   settled_times are refused; a ValueError push reaches no backend; times=True words and begins come through the double.
3. The ABI entry is exported, in the header and in the ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest

import fake_hip
from conftest import ROOT
from online_ref import CarriedDecode
from test_online_bigram_host import FakeOnlineBigramSession, dense_of, random_chunks, random_costs, whole, word_trans


@pytest.mark.parametrize("W", [17, 18, 19, 20])
def test_carried_bigram_recursion_equals_the_whole_decode_of_every_prefix(W):
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(1900 + W)
    n = 2 + W % 3
    skip = bool(W % 2) and n > 2
    B, init = random_costs(rng, W, 0.25)
    assert np.isinf(B).any() and np.isinf(init).any()                     # forbidden arcs, words that cannot start
    graph, _ = packed_bigram_lattice([word_trans(rng, n, skip) for _ in range(W)], n, B, init)
    nes = graph["row_state"] < 0
    trans, ends = dense_of(graph), graph["end_rows"]
    R = len(nes)
    assert R == 1 + W * n + W and len(ends) == W
    first = 1 + W * (n - 1) + W                                           # state 0 of word w is row first + w
    rw = np.where(nes, -1, graph["row_state"] // n)
    T = 14
    E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(R, T)))
    # a few cheap words that may start and follow each other, so that paths pass through several of the 17+ words
    cheap = rng.permutation(W)[:4]
    for k, wd in enumerate(cheap):
        E[np.flatnonzero(rw == wd), 3 * k:3 * k + 4] *= 0.1
    cd = CarriedDecode(nes, trans, ends)
    t, prefixes, seen_words = 0, 0, set()
    for c in [1] + random_chunks(rng, T - 1):                             # (the first push: exactly one frame)
        cd.push(E[:, t:t + c])
        t += c
        ec, bi, path = cd.result()
        if t == 1:
            # the carried form's own column 0: the start row at 0, first states hold init[w] + e, everything else is +inf
            want = np.full(R, np.inf)
            want[0] = 0.0
            want[first:first + W] = init + E[first:first + W, 0]
            np.testing.assert_array_equal(cd.col, want)
            assert len(path) == 0 and np.all(np.isinf(ec))
            continue
        if c == 0:
            continue
        ec_k, path_k = whole(E[:, :t], nes, trans, ends)
        np.testing.assert_array_equal(ec, ec_k)
        np.testing.assert_array_equal(path, path_k)
        prefixes += 1
        seen_words.update(int(rw[r]) for r, _ in path if rw[r] >= 0)
    assert t == T and prefixes >= 4 and len(seen_words) >= 2


# ----------------------------------------------------------------------------------------------------------------------
class Counted:
    made = 0                                          # sessions constructed, of either class


class FakeNarrowBigramSession(FakeOnlineBigramSession):
    def __init__(self, ctx, lat, n_streams, max_frames):
        Counted.made += 1
        super().__init__(ctx, lat, n_streams, max_frames)


class FakeBigramWideSession(FakeOnlineBigramSession):
    """Test double of `_hip.OnlineBigramWideSession`: (ctx, lat, n_streams, max_frames) and nothing else."""

    def __init__(self, ctx, lat, n_streams, max_frames):
        Counted.made += 1
        super().__init__(ctx, lat, n_streams, max_frames)

    def commit(self, *a, **k):
        raise AssertionError("the decoder must refuse before the session is asked")

    tail = commit


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineBigramSession", FakeNarrowBigramSession, raising=False)
    monkeypatch.setattr(_hip, "OnlineBigramWideSession", FakeBigramWideSession, raising=True)
    monkeypatch.setattr(Counted, "made", 0)
    for cls in (FakeNarrowBigramSession, FakeBigramWideSession):          # (`pushes` counts per class)
        monkeypatch.setattr(cls, "pushes", 0, raising=False)
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


def bigram_decoder(rng, hmms, forbid=0.2):
    from sr.recognition.batch import ContinuousDecoder
    B, init = random_costs(rng, len(hmms), forbid)
    return ContinuousDecoder(hmms, grammar="bigram", bigram=B, initial=init)


@pytest.mark.parametrize("W,wide,cls", [(17, True, FakeBigramWideSession), (20, True, FakeBigramWideSession),
                                        (10, True, FakeNarrowBigramSession), (10, False, FakeNarrowBigramSession),
                                        (16, True, FakeNarrowBigramSession), (17, False, FakeNarrowBigramSession)])
def test_online_bigram_routes_by_word_count_and_permission(fake_backend, W, wide, cls):
    """`wide=True` is a permission: beyond 16 words it gives the wide bigram session, up to 16 the narrow one as without
    it; without it the narrow session class is asked whatever the word count (the library refuses beyond 16)."""
    from sr.recognition.batch import OnlineBigramDecoder, OnlineDecoder
    rng = np.random.default_rng(50 + W)
    hmms, _ = make_models(rng, W)
    dec = bigram_decoder(rng, hmms)
    on = dec.online_bigram(n_streams=2, max_frames=8, wide=wide)
    assert type(on) is OnlineBigramDecoder and isinstance(on, OnlineDecoder) and type(on.session) is cls
    assert on.wide == (cls is FakeBigramWideSession) and on.settles is False
    assert on.max_frames == 8 == on.session.max_frames and on.window is None and Counted.made == 1
    # the keyword is the last positional argument of the class
    on2 = OnlineBigramDecoder(dec, 2, 8, None, None, None, False, False, wide)
    assert type(on2.session) is cls


def test_wide_bigram_decoder_refuses_window_and_settling(fake_backend):
    from sr.recognition import _hip
    rng = np.random.default_rng(51)
    hmms, utterance = make_models(rng, 17)
    dec = bigram_decoder(rng, hmms)
    for kw in (dict(window=10), dict(max_frames=10, settle=True), dict(window=10, settle=True)):
        with pytest.raises(_hip.Unsupported, match="not built yet"):
            dec.online_bigram(n_streams=2, wide=True, **kw)
    assert Counted.made == 0                                              # refused before a session is made
    for bad in (dict(n_streams=0, max_frames=10), dict(n_streams=3, max_frames=0), dict(n_streams=3), dict(n_streams=3, max_frames=5, window=5)):
        with pytest.raises(ValueError):
            dec.online_bigram(wide=True, **bad)
    assert Counted.made == 0
    on = dec.online_bigram(n_streams=3, max_frames=10, times=True, wide=True)
    assert on.settles is False
    on.push([1], [utterance([16, 0])[:6]])
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(_hip.Unsupported):
            call([1])
        with pytest.raises(_hip.Unsupported):
            call()
    assert on.frames.tolist() == [0, 6, 0]
    # a 10-word decoder keeps its window and its settled prefix with the keyword (today's route: the narrow class is asked
    # with window= / settle=, which this double does not take)
    hmms10, _ = make_models(rng, 10)
    dec10 = bigram_decoder(rng, hmms10)
    for kw in (dict(window=10), dict(max_frames=10, settle=True)):
        with pytest.raises(TypeError):
            dec10.online_bigram(n_streams=2, wide=True, **kw)
    # another grammar is refused as before
    from sr.recognition.batch import ContinuousDecoder
    with pytest.raises(_hip.Unsupported):
        ContinuousDecoder(hmms, grammar="loop").online_bigram(2, 10, wide=True)


def test_wide_bigram_decoder_refuses_a_bad_push_before_the_backend_is_touched(fake_backend):
    from sr.recognition import _hip
    rng = np.random.default_rng(52)
    hmms, _ = make_models(rng, 18)
    on = bigram_decoder(rng, hmms).online_bigram(n_streams=3, max_frames=10, wide=True)
    assert type(on.session) is FakeBigramWideSession
    x = rng.normal(size=(4, D_))
    on.push([2, 0], [x, x[:3]])
    before, calls = on.frames, FakeBigramWideSession.pushes
    assert before.tolist() == [3, 0, 4] and calls == 1
    for ids, chunks in (([1, 1], [x, x]),                                 # an id twice
                        ([0, 3], [x, x]), ([-1], [x]),                    # ids out of range
                        ([0], [rng.normal(size=(4, D_ + 1))]),            # another feature dimension
                        ([0], [x[0]]),                                    # not a [t, D] array
                        ([1, 2], [x, rng.normal(size=(7, D_))]),          # stream 2: 4 + 7 > 10 -- stream 1 must not move either
                        ([0, 1], [x])):                                   # chunks and ids do not pair up
        with pytest.raises(ValueError):
            on.push(ids, chunks)
        assert on.frames.tolist() == before.tolist() and FakeBigramWideSession.pushes == calls
    b = _hip.Batch(on.decoder.ctx, [rng.normal(size=(8, D_)), x])
    for ids, kw in (([1, 2], dict(first=[0, 2], count=[8, 3])), ([1, 2], dict(first=[-1, 0])), ([1, 2], dict(count=[8, 7])), ([2, 1], dict())):
        with pytest.raises(ValueError):
            on.push_batch(ids, b, **kw)
        assert on.frames.tolist() == before.tolist() and FakeBigramWideSession.pushes == calls
    with pytest.raises(ValueError):
        on.push_audio([0], [np.zeros(100, dtype=np.int16)])               # no front-end
    on.push_batch([1, 2], b, first=[2, 0], count=[6, 4])                  # exactly to capacity is fine
    assert on.frames.tolist() == [3, 6, 8]


def test_wide_bigram_decoder_results_and_word_times(fake_backend):
    """`result` of a 19-word bigram decoder in label and in path mode: the carried decode of the prefix, its begins what
    `path_to_word_times` gives for the path; finish frees the id."""
    from sr.recognition import _hip
    from sr.recognition.batch import path_to_word_times, path_to_words
    rng = np.random.default_rng(53)
    W = 19
    hmms, utterance = make_models(rng, W)
    dec = bigram_decoder(rng, hmms, forbid=0.0)
    on = dec.online_bigram(n_streams=4, max_frames=40, times=True, wide=True)
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


def test_header_binding_and_library_have_the_wide_bigram_entry(built_library):
    from sr.recognition import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmmhmm.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gh_online_create_bigram_wide\s*\(", text)
    assert "gh_online_create_bigram_wide" in _hip.SIGNATURES
    assert _hip.SIGNATURES["gh_online_create_bigram_wide"] == _hip.SIGNATURES["gh_online_create"]
    assert hasattr(ctypes.CDLL(built_library), "gh_online_create_bigram_wide")
    assert issubclass(_hip.OnlineBigramWideSession, _hip.OnlineSession)
    assert not issubclass(_hip.OnlineBigramWideSession, (_hip.OnlineBigramSession, _hip.OnlineWideSession))
