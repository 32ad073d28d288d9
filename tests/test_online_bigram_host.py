# -*- coding: utf-8 -*-
"""Online decoding with a bigram grammar on the host (no GPU).

1. The carried recursion (tests/online_ref.py) on `packed_bigram_lattice` graphs -- forbidden pairs, words that cannot
   start -- in random chunkings with 0-frame pushes: every prefix of >= 2 frames is BITWISE `O.decode_states` of that
   prefix (end costs and path).  A ONE-frame prefix is pinned against the carried form only: on these graphs every end
   row is +inf after one frame and the oracle's reference-style walk does not terminate there.
2. The reference's own G20 decodes fed in chunks of 1, 7 and 50 frames.
3. The host logic of `sr.recognition.batch.OnlineBigramDecoder` on a double of `_hip.OnlineBigramSession` that computes
   real results with `CarriedDecode`, and the export of `gh_online_create_bigram`."""
import ctypes
import warnings

import numpy as np
import pytest

import fake_hip
from conftest import load_golden
from online_ref import CarriedDecode
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


def random_costs(rng, W, forbid):
    """B [W, W] with a fraction `forbid` of +inf entries, every word keeping one way in; start costs with some +inf."""
    B = rng.uniform(0.0, 4.0, size=(W, W))
    B[rng.random((W, W)) < forbid] = np.inf
    B[rng.integers(0, W, size=W), np.arange(W)] = rng.uniform(0.0, 4.0, size=W)
    init = rng.uniform(0.0, 2.0, size=W)
    init[rng.random(W) < 0.3] = np.inf
    init[int(rng.integers(0, W))] = rng.uniform(0.0, 2.0)
    return B, init


def dense_of(graph):
    R = len(graph["row_state"])
    t = np.full((R, R), np.inf)
    t[graph["arc_to"], graph["arc_from"]] = graph["arc_cost"]
    return t


def whole(E, nes, trans, ends):
    """The oracle's whole decode with the end selection in column T - 1 (T >= 2)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        costs, path = O.decode_states(E, nes, trans, end_points=[[int(e), E.shape[1] - 1] for e in ends])
    return costs[np.asarray(ends), -1], np.asarray(path, dtype=np.int64).reshape(-1, 2)


def random_chunks(rng, T):
    """Chunk lengths 0 .. 4 that sum to T."""
    out = []
    while sum(out) < T:
        out.append(int(min(rng.integers(0, 5), T - sum(out))))
    if rng.random() < 0.5:
        out.append(0)
    return out


CASES = [(2, 2, False), (5, 3, True), (10, 5, False), (4, 8, True), (3, 12, False)]


@pytest.mark.parametrize("W,n,skip", CASES)
def test_carried_bigram_recursion_equals_the_whole_decode(W, n, skip):
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(9000 + 100 * W + n)
    prefixes = 0
    for rep in range(3):
        B, init = random_costs(rng, W, rng.uniform(0.1, 0.3))
        graph, _ = packed_bigram_lattice([word_trans(rng, n, skip) for _ in range(W)], n, B, init)
        nes = graph["row_state"] < 0
        trans, ends = dense_of(graph), graph["end_rows"]
        R = len(nes)
        first = 1 + W * (n - 1) + W                                       # state 0 of word w is row first + w
        T = (n - 1, 2 * n + 5, 3 * n + 9)[rep] if n > 2 else (2, 9, 14)[rep]   # (rep 0: shorter than any word)
        E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(R, T)))
        cd = CarriedDecode(nes, trans, ends)
        t = 0
        for c in random_chunks(rng, T):
            before = cd.t
            cd.push(E[:, t:t + c])
            t += c
            assert cd.t == t == before + c
            ec, bi, path = cd.result()
            if t == 0:
                assert bi == -1 and len(path) == 0 and np.all(np.isinf(ec))
            elif t == 1:
                # the carried form's own column 0: the start row at 0, first states hold init[w] + e, everything else is
                # +inf; no words
                want = np.full(R, np.inf)
                want[0] = 0.0
                want[first:first + W] = init + E[first:first + W, 0]
                np.testing.assert_array_equal(cd.col, want)
                assert np.all(np.isinf(ec)) and len(path) == 0
            else:
                ec_k, path_k = whole(E[:, :t], nes, trans, ends)
                np.testing.assert_array_equal(ec, ec_k)
                np.testing.assert_array_equal(path, path_k)
                prefixes += 1
        assert t == T
    assert prefixes >= 5                                                  # (the comparison above is not vacuous)


@pytest.mark.parametrize("chunk", [1, 7, 50])
def test_G20_in_chunks(chunk):
    """The reference's own decodes of the bigram graph (random, forbidden and tied costs), fed chunk by chunk: BIT-EXACT
    paths and digits."""
    g = load_golden("G20_bigram_grammar")
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
            cd = CarriedDecode(nes, trans, ends)
            cols = np.concatenate([cd.push(E[:, t:t + chunk]) for t in range(0, E.shape[1], chunk)], axis=1)
            np.testing.assert_allclose(cols, g[pp + "costs%d" % u], rtol=1e-12)
            _, _, path = cd.result()
            np.testing.assert_array_equal(path, g[pp + "path%d" % u])
            assert O.path_to_words(path, nes, rw) == list(g[pp + "digits%d" % u])


# ----------------------------------------------------------------------------------------------------------------------
class FakeOnlineBigramSession:
    """Test double of `_hip.OnlineBigramSession` on the carried recursion: same surface, the oracle's numbers."""
    pushes = 0                                        # calls that reached the backend (the ValueError tests watch it)

    def __init__(self, ctx, lat, n_streams, max_frames):
        from sr.recognition import _hip
        g = lat.graphs[0]
        W = len(g["end_rows"])
        if lat.L != 1 or np.sum(np.asarray(g["row_state"]) < 0) != 1 + W:
            raise _hip.Unsupported("the test double takes one bigram graph")
        self.lat, self.g = lat, g
        self.n_streams, self.max_frames = int(n_streams), int(max_frames)
        self.n_end = W
        nes = np.asarray(g["row_state"]) < 0
        self.streams = [CarriedDecode(nes, lat._dense(g), g["end_rows"]) for _ in range(self.n_streams)]

    def push(self, batch, ids, first=None, count=None):
        type(self).pushes += 1
        ids = np.asarray(ids, dtype=np.int64)
        assert len(ids) == batch.U == len(set(ids.tolist())) and ids.min() >= 0 and ids.max() < self.n_streams
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
        from sr.recognition import _hip
        raise _hip.Unsupported("a bigram session has no settled prefix")

    tail = commit

    def close(self):
        pass


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineBigramSession", FakeOnlineBigramSession, raising=False)
    monkeypatch.setattr(FakeOnlineBigramSession, "pushes", 0)
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
            Tw = int(rng.integers(N_, 2 * N_ + 3))
            st = np.minimum(np.arange(Tw) * N_ // Tw, N_ - 1)
            segs.append(means[wd, st, 0] + 0.5 * rng.normal(size=(Tw, D_)))
        return np.concatenate(segs)
    return hmms, utterance


def bigram_decoder(rng, hmms):
    from sr.recognition.batch import ContinuousDecoder
    B, init = random_costs(rng, W_, 0.2)
    return ContinuousDecoder(hmms, grammar="bigram", bigram=B, initial=init)


def test_online_bigram_result_is_the_carried_decode_of_the_prefix(fake_backend):
    """Interleaved subsets, streams that sit ticks out, finish and reuse of an id: at every point `result` of a stream is
    `path_to_words` / `path_to_word_times` of the carried path of what it has been given, in label and in path mode."""
    from sr.recognition import _hip
    from sr.recognition.batch import OnlineBigramDecoder, OnlineDecoder, path_to_word_times, path_to_words
    rng = np.random.default_rng(21)
    hmms, utterance = make_models(rng)
    dec = bigram_decoder(rng, hmms)
    on = dec.online_bigram(n_streams=5, max_frames=60, times=True)
    assert isinstance(on, OnlineBigramDecoder) and isinstance(on, OnlineDecoder) and on.max_frames == 60 and on.window is None
    g = dec.lat.graphs[0]
    nes = np.asarray(g["row_state"]) < 0
    utts = {k: utterance(rng.integers(0, W_, size=rng.integers(1, 4))) for k in range(5)}
    pos = {k: 0 for k in range(5)}
    words, info = on.result()                                            # nothing pushed yet
    assert words == [[]] * 5 and info["best_end"].tolist() == [-1] * 5 and np.all(np.isinf(info["end_cost"]))

    def check(ids):
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
        assert info["frames"].tolist() == [pos[k] for k in ids]

    reused = some_words = False
    for tick in range(60):
        live = [k for k in range(5) if pos[k] < len(utts[k])]
        if not live:
            break
        ids = [int(k) for k in rng.permutation(live)[:rng.integers(1, len(live) + 1)]]
        lens = [int(rng.integers(0, 6)) for _ in ids]                    # 0: the stream sits this tick out
        on.push(ids, [utts[k][pos[k]:pos[k] + c] for k, c in zip(ids, lens)])
        for k, c in zip(ids, lens):
            pos[k] = min(pos[k] + c, len(utts[k]))
        assert on.frames.tolist() == [pos[k] for k in range(5)]
        check([k for k in ids if pos[k] > 0])
        done = [k for k in ids if pos[k] == len(utts[k])]
        if done and not reused:                                          # an utterance ended: final result, id reused
            k = done[0]
            fw, fi = on.finish([k])
            some_words = len(fw[0]) >= 1
            assert on.frames[k] == 0
            utts[k], pos[k], reused = utterance([1, 2]), 0, True
    assert reused and some_words and all(pos[k] == len(utts[k]) for k in range(5))
    on.reset()
    assert on.frames.tolist() == [0] * 5
    on.close()


def test_online_bigram_refuses_before_the_backend_is_touched(fake_backend):
    from sr.recognition import _hip
    rng = np.random.default_rng(22)
    hmms, utterance = make_models(rng)
    dec = bigram_decoder(rng, hmms)
    for bad in (dict(n_streams=0, max_frames=10), dict(n_streams=3, max_frames=0), dict(n_streams=3, max_frames=None)):
        with pytest.raises(ValueError):
            dec.online_bigram(**bad)
    on = dec.online_bigram(n_streams=3, max_frames=10)
    x = rng.normal(size=(4, D_))
    on.push([2, 0], [x, x[:3]])
    before, calls = on.frames, FakeOnlineBigramSession.pushes
    assert before.tolist() == [3, 0, 4] and calls == 1
    for ids, chunks in (([1, 1], [x, x]),                                 # an id twice
                        ([0, 3], [x, x]), ([-1], [x]),                    # ids out of range
                        ([0], [rng.normal(size=(4, D_ + 1))]),            # another feature dimension
                        ([0], [x[0]]),                                    # not a [t, D] array
                        ([1, 2], [x, rng.normal(size=(7, D_))]),          # stream 2: 4 + 7 > 10 -- stream 1 must not move either
                        ([0, 1], [x])):                                   # chunks and ids do not pair up
        with pytest.raises(ValueError):
            on.push(ids, chunks)
        assert on.frames.tolist() == before.tolist() and FakeOnlineBigramSession.pushes == calls
    b = _hip.Batch(dec.ctx, [rng.normal(size=(8, D_)), x])
    for ids, kw in (([1, 2], dict(first=[0, 2], count=[8, 3])), ([1, 2], dict(first=[-1, 0])),   # outside the utterance
                    ([1, 2], dict(count=[8, 7])), ([2, 1], dict())):                             # ... and stream 2 past max_frames
        with pytest.raises(ValueError):
            on.push_batch(ids, b, **kw)
        assert on.frames.tolist() == before.tolist() and FakeOnlineBigramSession.pushes == calls
    with pytest.raises(ValueError):
        on.result([5])
    with pytest.raises(ValueError):
        on.reset([3])
    with pytest.raises(ValueError):                                       # no front-end, no endpointer
        on.push_audio([0], [np.zeros(100, dtype=np.int16)])
    on.push_batch([1, 2], b, first=[2, 0], count=[6, 4])                  # exactly to capacity is fine
    assert on.frames.tolist() == [3, 6, 8]
    # nothing settles
    for call in (on.commit, on.settled, on.settled_times):
        with pytest.raises(_hip.Unsupported):
            call([0])
    assert on.frames.tolist() == [3, 6, 8]


def test_online_bigram_needs_the_bigram_grammar(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    hmms, _ = make_models(np.random.default_rng(23))
    for dec in (ContinuousDecoder(hmms, grammar="loop"), ContinuousDecoder(hmms, n_layers=2)):
        with pytest.raises(_hip.Unsupported):
            dec.online_bigram(2, 10)
    assert FakeOnlineBigramSession.pushes == 0


def test_library_exports_the_bigram_entry(built_library):
    from sr.recognition import _hip
    lib = ctypes.CDLL(built_library)
    assert hasattr(lib, "gh_online_create_bigram")
    assert "gh_online_create_bigram" in _hip.SIGNATURES
    assert issubclass(_hip.OnlineBigramSession, _hip.OnlineSession)
