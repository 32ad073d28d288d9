# -*- coding: utf-8 -*-
"""Online decoding on the K-layer word lattice, on the host (no GPU).

1. The carried recursion (tests/online_ref.py) on `packed_lattice` graphs of 1 to 8 layers, fed in random chunks of 0 to 5
   frames: after every prefix of >= 2 frames end costs, chosen end and path are BITWISE `O.decode_states` of that prefix.
   A ONE-frame prefix is pinned against the carried form's own causal column 0: on a layer lattice the reference's column
   wrap (decode.py:109-114) reads the column being filled, so "the whole decode of one frame" is not what a stream that is
   still arriving can report.  This test passes without the feature: it pins the contract the kernel is held to.
2. The reference's own G4 decodes (K = 1, 2, 3, 7) fed in chunks of 1, 7 and 50 frames.
3. The host logic of `sr.recognition.batch.OnlineLayersDecoder` on a double of `_hip.OnlineLayersSession` that computes
   real results with `CarriedDecode`: routing, refusals before the backend is touched, results against `decode_batch`.
4. The ABI entry is exported, in the header and in the ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest

import fake_hip
from conftest import ROOT, load_golden
from online_ref import CarriedDecode
from oracle import ref_numpy as O
from test_online_bigram_host import FakeOnlineBigramSession, dense_of, whole, word_trans


def last_of_equal_minima(ec):
    best, bi = np.inf, -1
    for k, v in enumerate(ec):
        if best >= v:                                 # decode.py:129-134
            best, bi = v, k
    return bi


@pytest.mark.parametrize("W,n,K,skip", [(3, 2, 1, False), (2, 3, 2, True), (3, 4, 5, False), (2, 5, 8, True)])
def test_carried_layer_recursion_equals_the_whole_decode_of_every_prefix(W, n, K, skip):
    from sr.recognition.continuous_speech import packed_lattice
    rng = np.random.default_rng(4000 + 100 * W + 10 * n + K)
    graph, _ = packed_lattice([word_trans(rng, n, skip) for _ in range(W)], n, [list(range(W))] * K)
    nes = graph["row_state"] < 0
    trans, ends = dense_of(graph), graph["end_rows"]
    R, P = len(nes), W * n
    assert R == 1 + K * (P + 1) and len(ends) == W
    T = K * n + 6                                                         # the first prefixes are too short for K words
    E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(R, T)))
    cd = CarriedDecode(nes, trans, ends)
    chunks = [1]                                                          # (the first push: exactly one frame)
    while sum(chunks) < T:
        chunks.append(int(min(rng.integers(0, 6), T - sum(chunks))))
    chunks.append(0)
    assert 0 in chunks[:-1] or K == 1
    t = prefixes = finite = 0
    for c in chunks:
        cd.push(E[:, t:t + c])
        t += c
        ec, bi, path = cd.result()
        if t == 1:
            # the causal column 0: the start row at 0, the first states of layer 0 hold their emission (the entry arcs cost
            # 0), everything else is +inf; every end is +inf, the chosen end is the last of them, no words
            want = np.full(R, np.inf)
            want[0] = 0.0
            first = 1 + np.arange(W) * n
            want[first] = E[first, 0]
            np.testing.assert_array_equal(cd.col, want)
            assert np.all(np.isinf(ec)) and bi == W - 1 and len(path) == 0   # (an empty path: no words)
            continue
        ec_k, path_k = whole(E[:, :t], nes, trans, ends)
        np.testing.assert_array_equal(ec, ec_k)
        assert bi == last_of_equal_minima(ec_k)
        np.testing.assert_array_equal(path, path_k)
        prefixes += 1
        finite += bool(np.isfinite(ec).any())
    assert t == T and prefixes >= 3 and finite >= 1


@pytest.mark.parametrize("chunk", [1, 7, 50])
def test_G4_in_chunks(chunk):
    """The reference's own decodes of the K-layer lattice, fed chunk by chunk: BIT-EXACT paths and digits."""
    g = load_golden("G4_lattice_decode")
    means, vars_, w = g["means"], g["vars"], g["w"]
    for K in (1, 2, 3, 7):
        p = "K%d_" % K
        rw, rs, ends = g[p + "row_word"], g[p + "row_state"], g[p + "ends"]
        R = len(rw)
        nes = rw < 0
        trans = np.full((R, R), np.inf)
        trans[g[p + "arc_to"], g[p + "arc_from"]] = g[p + "arc_cost"]
        states = [None if nes[r] else (means[rw[r], rs[r]], vars_[rw[r], rs[r]], w[rw[r], rs[r]]) for r in range(R)]
        E = O.emission_matrix(g[p + "x"], states)
        cd = CarriedDecode(nes, trans, ends)
        cols = np.concatenate([cd.push(E[:, t:t + chunk]) for t in range(0, E.shape[1], chunk)], axis=1)
        np.testing.assert_allclose(cols, g[p + "costs"], rtol=1e-12)
        _, _, path = cd.result()
        np.testing.assert_array_equal(path, g[p + "path"])
        assert O.path_to_words(path, nes, rw) == list(g[p + "digits"])


# ----------------------------------------------------------------------------------------------------------------------
class FakeOnlineLayersSession(FakeOnlineBigramSession):
    """Test double of `_hip.OnlineLayersSession` on the carried recursion: (ctx, lat, n_streams, max_frames) and nothing
    else, the oracle's numbers; `commit` and `tail` must never be reached through the decoder."""
    made = 0

    def __init__(self, ctx, lat, n_streams, max_frames):
        from sr.recognition import _hip
        type(self).made += 1
        g = lat.graphs[0]
        W = len(g["end_rows"])
        if lat.L != 1 or (len(g["row_state"]) - 1) % (np.sum(np.asarray(g["row_state"]) < 0) - 1) != 0:
            raise _hip.Unsupported("the test double takes one K-layer lattice")
        self.lat, self.g = lat, g
        self.n_streams, self.max_frames = int(n_streams), int(max_frames)
        self.n_end = W
        nes = np.asarray(g["row_state"]) < 0
        self.streams = [CarriedDecode(nes, lat._dense(g), g["end_rows"]) for _ in range(self.n_streams)]

    def commit(self, *a, **k):
        raise AssertionError("the decoder must refuse before the session is asked")

    tail = commit


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineLayersSession", FakeOnlineLayersSession, raising=False)
    monkeypatch.setattr(FakeOnlineLayersSession, "pushes", 0, raising=False)
    monkeypatch.setattr(FakeOnlineLayersSession, "made", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


W_, N_, M_, D_, K_ = 4, 3, 2, 3, 3


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
            Tw = int(rng.integers(N_, 2 * N_ + 3))
            st = np.minimum(np.arange(Tw) * N_ // Tw, N_ - 1)
            segs.append(means[wd, st, 0] + 0.5 * rng.normal(size=(Tw, D_)))
        return np.concatenate(segs)
    return hmms, utterance


def test_online_layers_routes_and_refuses_before_the_backend_is_touched(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder, OnlineDecoder, OnlineLayersDecoder
    rng = np.random.default_rng(31)
    hmms, utterance = make_models(rng)
    # another grammar
    bigram = ContinuousDecoder(hmms, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(W_, W_)))
    for dec, hint in ((ContinuousDecoder(hmms, grammar="loop"), "online takes it"), (bigram, "online_bigram takes it")):
        with pytest.raises(_hip.Unsupported, match=hint):
            dec.online_layers(2, 10)
    dec = ContinuousDecoder(hmms, n_layers=K_)
    assert dec.grammar == "layers" and dec._max_labels(100) == K_ + 1
    # no window, no settling: the keywords do not exist
    for kw in (dict(window=10), dict(settle=True)):
        with pytest.raises(TypeError):
            dec.online_layers(2, 10, **kw)
    for bad in (dict(n_streams=0, max_frames=10), dict(n_streams=3, max_frames=0), dict(n_streams=3, max_frames=None)):
        with pytest.raises(ValueError):
            dec.online_layers(**bad)
    assert FakeOnlineLayersSession.made == 0                              # refused before a session is made
    # the other two entry points keep refusing the layers decoder, and name the one that takes it
    with pytest.raises(_hip.Unsupported, match="online_layers takes it"):
        dec.online(2, 10)
    with pytest.raises(_hip.Unsupported, match="online_layers takes it"):
        dec.online_bigram(2, 10)
    on = dec.online_layers(n_streams=3, max_frames=10, times=True)
    assert type(on) is OnlineLayersDecoder and isinstance(on, OnlineDecoder) and type(on.session) is FakeOnlineLayersSession
    assert on.max_frames == 10 == on.session.max_frames and on.window is None and on.settles is False and on.wide is False
    assert FakeOnlineLayersSession.made == 1
    x = rng.normal(size=(4, D_))
    on.push([2, 0], [x, x[:3]])
    before, calls = on.frames, FakeOnlineLayersSession.pushes
    assert before.tolist() == [3, 0, 4] and calls == 1
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(_hip.Unsupported):
            call([0])
        with pytest.raises(_hip.Unsupported):
            call()
    for ids, chunks in (([1, 1], [x, x]),                                 # an id twice
                        ([0, 3], [x, x]), ([-1], [x]),                    # ids out of range
                        ([0], [rng.normal(size=(4, D_ + 1))]),            # another feature dimension
                        ([0], [x[0]]),                                    # not a [t, D] array
                        ([1, 2], [x, rng.normal(size=(7, D_))]),          # stream 2: 4 + 7 > 10 -- stream 1 must not move either
                        ([0, 1], [x])):                                   # chunks and ids do not pair up
        with pytest.raises(ValueError):
            on.push(ids, chunks)
        assert on.frames.tolist() == before.tolist() and FakeOnlineLayersSession.pushes == calls
    b = _hip.Batch(dec.ctx, [rng.normal(size=(8, D_)), x])
    for ids, kw in (([1, 2], dict(first=[0, 2], count=[8, 3])), ([1, 2], dict(first=[-1, 0])),   # outside the utterance
                    ([1, 2], dict(count=[8, 7])), ([2, 1], dict()), ([1, 1], dict())):           # past max_frames; an id twice
        with pytest.raises(ValueError):
            on.push_batch(ids, b, **kw)
        assert on.frames.tolist() == before.tolist() and FakeOnlineLayersSession.pushes == calls
    with pytest.raises(ValueError):
        on.result([5])
    with pytest.raises(ValueError):
        on.reset([3])
    with pytest.raises(ValueError):                                       # no front-end, no endpointer
        on.push_audio([0], [np.zeros(100, dtype=np.int16)])
    on.push_batch([1, 2], b, first=[2, 0], count=[6, 4])                  # exactly to capacity is fine
    assert on.frames.tolist() == [3, 6, 8]


@pytest.mark.parametrize("times", [False, True])
def test_online_layers_result_is_decode_batch_of_what_was_pushed(fake_backend, times):
    """Interleaved subsets, streams that sit ticks out, finish and reuse of an id: from two frames on `result` of a stream
    is `decode_batch` of what it has been given -- words, end costs, chosen end, paths, and with times=True the begins; a
    one-frame stream reports the carried column 0 and no words."""
    from sr.recognition import _hip
    rng = np.random.default_rng(32 + times)
    hmms, utterance = make_models(rng)
    from sr.recognition.batch import ContinuousDecoder
    dec = ContinuousDecoder(hmms, n_layers=K_)
    on = dec.online_layers(n_streams=5, max_frames=60, times=times)
    g = dec.lat.graphs[0]
    nes = np.asarray(g["row_state"]) < 0
    utts = {k: utterance(rng.integers(0, W_, size=K_)) for k in range(5)}
    pos = {k: 0 for k in range(5)}
    words, info = on.result()                                             # nothing pushed yet
    assert words == [[]] * 5 and info["best_end"].tolist() == [-1] * 5 and np.all(np.isinf(info["end_cost"]))
    seen = dict(one=0, short=0, full=0)

    def check(ids):
        words, info = on.result(ids)
        wp, ip = on.result(ids, want_path=True)
        assert info["frames"].tolist() == [pos[k] for k in ids] and words == wp
        for u, k in enumerate(ids):
            if pos[k] == 1:
                b = _hip.Batch(dec.ctx, [utts[k][:1]])
                b.loglik(dec.gmm, fetch=False)
                cd = CarriedDecode(nes, dec.lat._dense(g), g["end_rows"])
                cd.push(dec.lat._emissions(b, 0, g)[0])
                np.testing.assert_array_equal(info["end_cost"][u], cd.result()[0])
                assert info["best_end"][u] == cd.result()[1] == W_ - 1
                assert words[u] == [] and len(ip["paths"][u]) == 0
                seen["one"] += 1
                continue
            b = _hip.Batch(dec.ctx, [utts[k][:pos[k]]])
            kw = dict(want_times=True) if times else {}
            ref_words, ref = dec.decode_batch(b, want_path=True, **kw)
            np.testing.assert_array_equal(info["end_cost"][u], ref["end_cost"][0])
            assert info["best_end"][u] == ref["best_end"][0] == ip["best_end"][u]
            np.testing.assert_array_equal(ip["paths"][u], ref["paths"][0])
            assert words[u] == ref_words[0]
            if times:
                assert info["begins"][u].tolist() == ref["begins"][0].tolist() == ip["begins"][u].tolist()
            if np.isfinite(ref["end_cost"][0]).any():
                assert len(words[u]) == K_
                seen["full"] += 1
            else:
                seen["short"] += 1

    reused = False
    for tick in range(80):
        live = [k for k in range(5) if pos[k] < len(utts[k])]
        if not live:
            break
        ids = [int(k) for k in rng.permutation(live)[:rng.integers(1, len(live) + 1)]]
        lens = [1 if pos[k] == 0 and k % 2 else int(rng.integers(0, 6)) for k in ids]   # (odd streams: a first push of one frame)
        on.push(ids, [utts[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)])
        for k, c in zip(ids, lens):
            pos[k] = min(pos[k] + c, len(utts[k]))
        assert on.frames.tolist() == [pos[k] for k in range(5)]
        check([k for k in ids if pos[k] > 0])
        done = [k for k in ids if pos[k] == len(utts[k])]
        if done and not reused:                                           # an utterance ended: final result, id reused
            k = done[0]
            fw, fi = on.finish([k])
            assert len(fw[0]) == K_ and on.frames[k] == 0
            utts[k], pos[k], reused = utterance([1, 2, 0]), 0, True
    assert reused and all(pos[k] == len(utts[k]) for k in range(5))
    assert seen["one"] >= 1 and seen["short"] >= 1 and seen["full"] >= 5
    on.reset()
    assert on.frames.tolist() == [0] * 5
    on.close()


def test_header_binding_and_library_have_the_layers_entry(built_library):
    from sr.recognition import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmmhmm.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gh_online_create_layers\s*\(", text)
    assert "gh_online_create_layers" in _hip.SIGNATURES
    assert _hip.SIGNATURES["gh_online_create_layers"] == _hip.SIGNATURES["gh_online_create"]
    assert hasattr(ctypes.CDLL(built_library), "gh_online_create_layers")
    assert issubclass(_hip.OnlineLayersSession, _hip.OnlineSession)
    assert not issubclass(_hip.OnlineLayersSession, (_hip.OnlineBigramSession, _hip.OnlineWideSession, _hip.OnlineBigramWideSession))
