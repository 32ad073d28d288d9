# -*- coding: utf-8 -*-
"""Online decoding on the host (no GPU).

1. The carried recursion (tests/online_ref.py: one column + the back-pointers) against the oracle's whole decode on
   `O.loop_grammar` graphs: random chunkings with 0- and 1-frame chunks, every carried column BITWISE the whole decode's,
   the result after k frames bitwise `O.decode_states` of the first k frames (k = 1, 2 included), and the reference's own
   G14 decodes fed in chunks.
2. The host logic of `sr.recognition.batch.OnlineDecoder` on the oracle-backed test double of the binding
   (tests/fake_hip.py, plus a double of `_hip.OnlineSession` built on online_ref.py): id bookkeeping, interleaved
   subsets, finish / reuse of an id, and every ValueError -- raised before the backend is touched, no stream moved."""
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


def whole(E, nes, trans, ends):
    """The oracle's whole decode with the end selection in column T - 1 (named as such: at T == 1 the reference's own
    spelling, column -1, never meets its `j != 0` stop)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        costs, path = O.decode_states(E, nes, trans, end_points=[[e, E.shape[1] - 1] for e in ends])
    ec = costs[np.asarray(ends), -1]
    best, bi = np.inf, -1
    for k, v in enumerate(ec):
        if best >= v:
            best, bi = v, k
    return costs, ec, bi, np.asarray(path, dtype=np.int64).reshape(-1, 2)


def words_of(path, nes, rw):
    return O.path_to_words(path, nes, rw) if len(path) else []


def random_chunks(rng, T):
    """Chunk lengths 0 .. 4 that sum to T."""
    out = []
    while sum(out) < T:
        out.append(int(min(rng.integers(0, 5), T - sum(out))))
    if rng.random() < 0.5:
        out.append(0)
    return out


@pytest.mark.parametrize("seed", range(20))
def test_carried_recursion_equals_the_whole_decode(seed):
    rng = np.random.default_rng(4000 + seed)
    W, n = int(rng.integers(1, 6)), int(rng.integers(2, 7))
    skip = bool(seed % 2)
    nes, rw, rs, trans, ends = O.loop_grammar([word_trans(rng, n, skip) for _ in range(W)], n, float(rng.choice([0.0, 0.7, 2.5])))
    R = len(nes)
    T = int(rng.integers(1, 40)) if seed > 2 else seed + 1            # (T = 1, 2, 3 among them)
    E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(R, T)))
    if seed % 5 == 0:
        E[rng.integers(1, R), rng.integers(0, T)] = np.inf            # an emission that underflowed
    full_costs = whole(E, nes, trans, ends)[0]
    cd = CarriedDecode(nes, trans, ends)
    t = 0
    for c in random_chunks(rng, T):
        cols = cd.push(E[:, t:t + c])
        np.testing.assert_array_equal(cols, full_costs[:, t:t + c])          # bitwise, column by column
        t += c
        assert cd.t == t
        if t == 0:
            ec, bi, path = cd.result()
            assert bi == -1 and len(path) == 0 and np.all(np.isinf(ec))
            continue
        _, ec_k, bi_k, path_k = whole(E[:, :t], nes, trans, ends)             # the whole decode of the PREFIX
        ec, bi, path = cd.result()
        np.testing.assert_array_equal(ec, ec_k)
        assert bi == bi_k
        np.testing.assert_array_equal(path, path_k)
        assert words_of(path, nes, rw) == words_of(path_k, nes, rw)
    assert t == T


@pytest.mark.parametrize("k", [1, 2])
def test_result_after_one_and_two_frames(k):
    """The reference's column wrap at c == 0 (decode.py:109-114) reads the column being filled when there is ONE frame:
    in a loop grammar that changes nothing, the carried form (which reads +inf there) gives the same cells."""
    rng = np.random.default_rng(7 + k)
    for W, n in ((1, 2), (3, 5), (10, 5), (4, 3)):
        nes, rw, rs, trans, ends = O.loop_grammar([word_trans(rng, n, True) for _ in range(W)], n, 0.5)
        E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 9.0, size=(len(nes), k)))
        costs, ec_k, bi_k, path_k = whole(E, nes, trans, ends)
        cd = CarriedDecode(nes, trans, ends)
        for c in range(k):
            np.testing.assert_array_equal(cd.push(E[:, c:c + 1])[:, 0], costs[:, c])
        ec, bi, path = cd.result()
        np.testing.assert_array_equal(ec, ec_k)
        assert bi == bi_k
        np.testing.assert_array_equal(path, path_k)


@pytest.mark.parametrize("chunk", [1, 7, 50])
def test_G14_in_chunks(chunk):
    """The reference's own decodes of the loop graph, fed chunk by chunk: its cost matrix, BIT-EXACT path and digits."""
    g = load_golden("G14_loop_grammar")
    means, vars_, w, wt = g["means"], g["vars"], g["w"], g["word_trans"]
    W, n = means.shape[:2]
    for pen in (0, 1):
        pp = "p%d_" % pen
        nes, rw, rs, trans, ends = O.loop_grammar([wt] * W, n, float(g[pp + "penalty"]))
        states = [None if nes[r] else (means[rw[r], rs[r]], vars_[rw[r], rs[r]], w[rw[r], rs[r]]) for r in range(len(rw))]
        for u in range(int(g["n_utts"])):
            E = O.emission_matrix(g[pp + "x%d" % u], states)
            cd = CarriedDecode(nes, trans, ends)
            cols = np.concatenate([cd.push(E[:, t:t + chunk]) for t in range(0, E.shape[1], chunk)], axis=1)
            np.testing.assert_allclose(cols, g[pp + "costs%d" % u], rtol=1e-12)
            ec, bi, path = cd.result()
            np.testing.assert_array_equal(path, g[pp + "path%d" % u])
            assert O.path_to_words(path, nes, rw) == list(g[pp + "digits%d" % u])


# ----------------------------------------------------------------------------------------------------------------------
class FakeOnlineSession:
    """Test double of `_hip.OnlineSession` on the carried recursion: same surface, the oracle's numbers."""
    pushes = 0                                        # calls that reached the backend (the ValueError tests watch it)

    def __init__(self, ctx, lat, n_streams, max_frames):
        from sr.recognition import _hip
        g = lat.graphs[0]
        if lat.L != 1 or np.sum(np.asarray(g["row_state"]) < 0) != 2:
            raise _hip.Unsupported("the test double takes one loop graph")
        self.lat, self.g = lat, g
        self.n_streams, self.max_frames = int(n_streams), int(max_frames)
        self.n_end = len(g["end_rows"])
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

    def result(self, ids=None, row_label=None, max_labels=None, want_path=False):
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        res = [self.streams[int(k)].result() for k in ids]
        out = dict(end_cost=np.array([r[0] for r in res]).reshape(len(ids), self.n_end),
                   best_end=np.array([r[1] for r in res], dtype=np.int32), frames=self.frames()[ids])
        if row_label is not None:
            rl = np.asarray(row_label)
            out["labels"] = [np.array(O.path_to_words(r[2], rl < 0, rl) if len(r[2]) else [], dtype=np.int32) for r in res]
        if want_path:
            out["paths"] = [r[2] for r in res]
        return out

    def close(self):
        pass


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "OnlineSession", FakeOnlineSession, raising=False)
    monkeypatch.setattr(FakeOnlineSession, "pushes", 0)
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


def test_online_decoder_bookkeeping(fake_backend):
    """Interleaved subsets in shuffled id order, streams that sit ticks out, finish and reuse of an id: at every point the
    running result of a stream is `decode_batch` of what it has been given."""
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(11)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=0.4)
    on = dec.online(n_streams=5, max_frames=60)
    utts = {k: utterance(rng.integers(0, W_, size=rng.integers(1, 4))) for k in range(5)}
    pos = {k: 0 for k in range(5)}
    assert on.frames.tolist() == [0] * 5
    words, info = on.result()                                            # nothing pushed yet
    assert words == [[]] * 5 and info["best_end"].tolist() == [-1] * 5 and np.all(np.isinf(info["end_cost"]))

    def check(ids):
        if not len(ids):
            return
        b = _hip.Batch(dec.ctx, [utts[k][:pos[k]] for k in ids])
        ref_words, ref = dec.decode_batch(b, want_path=True)
        words, info = on.result(ids)
        wp, ip = on.result(ids, want_path=True)
        assert words == ref_words == wp
        np.testing.assert_array_equal(info["best_end"], ref["best_end"])
        np.testing.assert_array_equal(info["end_cost"].reshape(-1), ref["end_cost_flat"])
        assert info["frames"].tolist() == [pos[k] for k in ids]
        for p, q in zip(ip["paths"], ref["paths"]):
            np.testing.assert_array_equal(p, q)

    reused = False
    for tick in range(40):
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
            b = _hip.Batch(dec.ctx, [utts[k]])
            assert fw == dec.decode_batch(b)[0]
            assert on.frames[k] == 0
            utts[k], pos[k], reused = utterance([1, 2]), 0, True
    assert reused and all(pos[k] == len(utts[k]) for k in range(5))
    on.reset()
    assert on.frames.tolist() == [0] * 5
    on.close()


def test_online_decoder_refuses_before_the_backend_is_touched(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(12)
    hmms, utterance = make_models(rng)
    dec = ContinuousDecoder(hmms, grammar="loop")
    on = dec.online(n_streams=3, max_frames=10)
    x = rng.normal(size=(4, D_))
    on.push([2, 0], [x, x[:3]])
    before, calls = on.frames, FakeOnlineSession.pushes
    assert before.tolist() == [3, 0, 4] and calls == 1
    for ids, chunks in (([1, 1], [x, x]),                                 # an id twice
                        ([0, 3], [x, x]), ([-1], [x]),                    # ids out of range
                        ([0], [rng.normal(size=(4, D_ + 1))]),            # another feature dimension
                        ([0], [x[0]]),                                    # not a [t, D] array
                        ([1, 2], [x, rng.normal(size=(7, D_))]),          # stream 2: 4 + 7 > 10 -- stream 1 must not move either
                        ([0, 1], [x])):                                   # chunks and ids do not pair up
        with pytest.raises(ValueError):
            on.push(ids, chunks)
        assert on.frames.tolist() == before.tolist() and FakeOnlineSession.pushes == calls
    b = _hip.Batch(dec.ctx, [rng.normal(size=(8, D_)), x])
    for ids, kw in (([1, 2], dict(first=[0, 2], count=[8, 3])), ([1, 2], dict(first=[-1, 0])),   # outside the utterance
                    ([1, 2], dict(count=[8, 7])), ([2, 1], dict())):                             # ... and stream 2 past max_frames
        with pytest.raises(ValueError):
            on.push_batch(ids, b, **kw)
        assert on.frames.tolist() == before.tolist() and FakeOnlineSession.pushes == calls
    with pytest.raises(ValueError):
        on.push_batch([1, 1], b)
    with pytest.raises(ValueError):
        on.result([5])
    with pytest.raises(ValueError):
        on.reset([3])
    on.push_batch([1, 2], b, first=[2, 0], count=[6, 4])                  # exactly to capacity is fine
    assert on.frames.tolist() == [3, 6, 8]
    on.push([0], [np.zeros((0, D_))])                                     # an empty tick never reaches the backend
    assert FakeOnlineSession.pushes == calls + 1


def test_online_needs_the_loop_grammar(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    hmms, _ = make_models(np.random.default_rng(13))
    with pytest.raises(_hip.Unsupported):
        ContinuousDecoder(hmms, n_layers=2).online(2, 10)
    with pytest.raises(_hip.Unsupported):
        ContinuousDecoder(hmms, grammar="bigram", bigram=np.zeros((W_, W_))).online(2, 10)
