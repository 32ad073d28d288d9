# -*- coding: utf-8 -*-
"""Online isolated-word recognition on the host (no GPU).

1. What the carried sweep computes, restated with `online_ref.CarriedDecode` (one per word chain): fed in random chunks
   (0- and 1-frame chunks among them) the carried column after k frames is column k - 1 of the reference's stored decode
   (G3 `costs_u_w`, 1e-12) and the last end cost is `evaluate_u[w]`; on random chains of 1, 2, 3, 5 and 8 states, with and
   without skip arcs, every prefix of k >= 2 frames is BITWISE `O.decode_states` of those k frames.  At k = 1 the carried
   column is the causal column 0 (start row: its emission, all others +inf), and that is NOT the reference's one-frame
   decode (its column wrap, decode.py:109-114, lets row r read row r - 1 of the same column): pinned, with the difference.
2. The host logic of `OnlineWordRecognizer` on a test double of `_hip.WordStreamSession` with the restatement as the backend."""
import warnings

import numpy as np
import pytest

import audio_capture_ref as A
import fake_hip
import stream_endpoints_ref as S
from conftest import load_golden
from online_ref import CarriedDecode
from oracle import ref_numpy as O
from stream_frontend_ref import FakeStreamFrontend, raw_stack
from test_online_host import word_trans


def random_chunks(rng, T):
    """Chunk lengths 0 .. 4 that sum to T (every run has 0- and 1-frame chunks with near certainty; the G3 test asserts it)."""
    out = []
    while sum(out) < T:
        out.append(int(min(rng.integers(0, 5), T - sum(out))))
    return out + [0]


def whole_decode(E, trans):
    """The oracle's decode of one chain (start row 0, end row n - 1), the end named in column T - 1."""
    n, T = E.shape
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        costs, _ = O.decode_states(E, np.zeros(n, dtype=bool), trans, end_points=[[n - 1, T - 1]])
    return costs


# ------------------------------------------------------------------ 1: the restatement
@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_carried_chains_reproduce_G3_in_random_chunks(tag):
    g = load_golden("G3_isolated_decode_" + tag)
    means, vars_, w, trans = g["means"], g["vars"], g["w"], g["trans"]
    W, n = means.shape[:2]
    rng = np.random.default_rng(31)
    seen = set()
    for u in range(len(g["words"])):
        x = g["x%d" % u]
        ends = []
        for i in range(W):
            E = O.emission_matrix(x, [(means[i, s], vars_[i, s], w[i, s]) for s in range(n)])
            ref = g["costs_%d_%d" % (u, i)]
            cd = CarriedDecode(np.zeros(n, dtype=bool), trans, [n - 1])
            t = 0
            for c in random_chunks(rng, E.shape[1]):
                seen.add(c)
                cols = cd.push(E[:, t:t + c])
                t += c
                if t >= 2 and c:                    # (k = 1 is the causal column: the next test)
                    np.testing.assert_array_equal(np.isinf(cd.col), np.isinf(ref[:, t - 1]))
                    fin = ~np.isinf(cd.col)
                    np.testing.assert_allclose(cd.col[fin], ref[fin, t - 1], rtol=1e-12)
                    assert cols.shape == (n, c)
            assert t == E.shape[1]
            ends.append(cd.result()[0][0])
        np.testing.assert_allclose(ends, g["evaluate_%d" % u], rtol=1e-12)
        assert int(np.argmin(ends)) == int(g["words"][u])
    assert {0, 1} <= seen


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_every_prefix_of_two_or_more_frames_is_the_whole_decode_bitwise(n, skip):
    rng = np.random.default_rng(100 * n + skip)
    for rep in range(4):
        trans = word_trans(rng, n, skip)
        T = int(rng.integers(2, 30))
        E = rng.uniform(0.5, 9.0, size=(n, T))
        if rep == 3:
            E[rng.integers(0, n), rng.integers(0, T)] = np.inf            # an emission that underflowed
        cd = CarriedDecode(np.zeros(n, dtype=bool), trans, [n - 1])
        t = 0
        for c in random_chunks(rng, T):
            cd.push(E[:, t:t + c])
            t += c
            if t >= 2:
                ref = whole_decode(E[:, :t], trans)
                np.testing.assert_array_equal(cd.col, ref[:, -1])
                np.testing.assert_array_equal(cd.result()[0], ref[-1:, -1])
        assert t == T


def test_one_frame_is_the_causal_column_and_not_the_one_frame_decode():
    rng = np.random.default_rng(17)
    differ = 0
    for n in (1, 2, 3, 5, 8):
        for skip in (False, True):
            trans = word_trans(rng, n, skip)
            E = rng.uniform(0.5, 9.0, size=(n, 3))
            cd = CarriedDecode(np.zeros(n, dtype=bool), trans, [n - 1])
            cd.push(E[:, :1])
            want = np.full(n, np.inf)
            want[0] = E[0, 0]
            np.testing.assert_array_equal(cd.col, want)                     # column 0 of every longer decode ...
            np.testing.assert_array_equal(cd.col, whole_decode(E, trans)[:, 0])
            np.testing.assert_array_equal(cd.col, whole_decode(E[:, :2], trans)[:, 0])
            one = whole_decode(E[:, :1], trans)[:, 0]                       # ... and not the reference's one-frame decode
            differ += int(not np.array_equal(one, cd.col))
            if n == 1:
                np.testing.assert_array_equal(one, cd.col)                  # (a one-state word has nothing to wrap into)
    assert differ >= 1


# ------------------------------------------------------------------ 2: host logic on a double of _hip.WordStreamSession
class FakeWordStreamSession:
    """Test double of `_hip.WordStreamSession` on the carried recursion: same surface, the oracle's numbers."""
    pushes = 0                                        # calls that reached the backend (the ValueError tests watch it)

    def __init__(self, ctx, lat, n_streams):
        g = lat.graphs[0]
        starts, ends = sorted(int(s) for s in g["start_rows"]), [int(e) for e in g["end_rows"]]
        R = len(g["row_state"])
        assert lat.L == 1 and len(starts) == len(ends) and not np.any(np.asarray(g["row_state"]) < 0)
        self.lat, self.g, self.n_streams = lat, g, int(n_streams)
        self.bounds = list(zip(starts, starts[1:] + [R]))
        assert all(lo <= e < hi for (lo, hi), e in zip(self.bounds, ends))
        dense = lat._dense(g)
        self.streams = [[CarriedDecode(np.zeros(hi - lo, dtype=bool), dense[lo:hi, lo:hi], [e - lo])
                         for (lo, hi), e in zip(self.bounds, ends)] for _ in range(self.n_streams)]

    def push(self, batch, ids, first=None, count=None):
        type(self).pushes += 1
        ids = np.asarray(ids, dtype=np.int64)
        assert len(ids) == batch.U == len(set(ids.tolist())) and ids.min() >= 0 and ids.max() < self.n_streams
        first = np.zeros(batch.U, dtype=np.int64) if first is None else np.asarray(first)
        count = batch.lengths - first if count is None else np.asarray(count)
        for u, k in enumerate(ids):
            E, _ = self.lat._emissions(batch, u, self.g)
            for cd, (lo, hi) in zip(self.streams[k], self.bounds):
                cd.push(E[lo:hi, first[u]:first[u] + count[u]])

    def reset(self, ids=None):
        for k in (range(self.n_streams) if ids is None else ids):
            for cd in self.streams[int(k)]:
                cd.reset()

    def frames(self):
        return np.array([s[0].t for s in self.streams], dtype=np.int64)

    def result(self, ids=None):
        ids = np.arange(self.n_streams) if ids is None else np.asarray(ids, dtype=np.int64)
        costs = np.array([[cd.result()[0][0] for cd in self.streams[int(k)]] for k in ids]).reshape(len(ids), len(self.bounds))
        T = self.frames()[ids]
        return dict(costs=costs, best=np.where(T > 0, np.argmin(costs, axis=1), -1).astype(np.int32), frames=T)

    def close(self):
        pass


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "WordStreamSession", FakeWordStreamSession, raising=False)
    monkeypatch.setattr(_hip, "StreamFrontend", FakeStreamFrontend, raising=False)
    monkeypatch.setattr(_hip, "EndpointStream", S.FakeEndpointStream, raising=False)
    monkeypatch.setattr(FakeWordStreamSession, "pushes", 0)
    monkeypatch.setattr(FakeStreamFrontend, "pushes", 0)
    monkeypatch.setattr(S.FakeEndpointStream, "pushes", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


W_, N_, M_ = 4, 3, 2


def make_recognizer(rng, D=3, use_gmm=True):
    import sr.recognition as R
    from sr.recognition.batch import IsolatedWordRecognizer
    hmms = []
    for i in range(W_):
        h = R.HMM(N_)
        mean, var = rng.normal(size=(N_, M_, D)) * 3.0, rng.uniform(0.5, 1.5, size=(N_, M_, D)) * (1.0 if D == 3 else 40.0)
        h.mu, h.sigma = mean[:, 0].copy(), var[:, 0].copy()
        h.use_gmm = use_gmm
        h.gmm_states = None
        if use_gmm:
            h.gmm_states = []
            for s in range(N_):
                g = R.GMM(mean[s, 0].copy(), var[s, 0].copy(), M_)
                g.update_models(mean[s], var[s], rng.dirichlet(np.ones(M_)))
                h.gmm_states.append(g)
        h.transitions = word_trans(rng, N_)
        hmms.append(h)
    return IsolatedWordRecognizer(hmms)


def test_online_recognizer_bookkeeping(fake_backend):
    """Interleaved subsets in shuffled id order, streams that sit ticks out, finish and reuse of an id: from two frames on
    the running result of a stream is `recognize` of what it has been given."""
    from sr.recognition.batch import OnlineWordRecognizer
    import sr.recognition.batch as B
    assert "OnlineWordRecognizer" in B.__all__
    rng = np.random.default_rng(21)
    rec = make_recognizer(rng)
    on = rec.online(n_streams=5)
    assert isinstance(on, OnlineWordRecognizer)
    utts = {k: rng.normal(size=(int(rng.integers(6, 20)), 3)) * 2.0 for k in range(5)}
    pos = {k: 0 for k in range(5)}
    words, info = on.result()                                            # nothing pushed yet
    assert words.dtype == np.int64 and words.tolist() == [-1] * 5 and np.all(np.isinf(info["costs"])) and info["costs"].shape == (5, W_)

    def check(ids):
        ids = [k for k in ids if pos[k] >= 2]
        if not ids:
            return
        ref_words, ref_costs = rec.recognize([utts[k][:pos[k]] for k in ids])
        words, info = on.result(ids)
        np.testing.assert_array_equal(words, ref_words)
        np.testing.assert_array_equal(info["costs"], ref_costs)
        assert info["frames"].tolist() == [pos[k] for k in ids]

    reused = False
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
        check(ids)
        done = [k for k in ids if pos[k] == len(utts[k])]
        if done and not reused:                                          # an utterance ended: final result, id reused
            k = done[0]
            fw, fi = on.finish([k])
            rw, rc = rec.recognize([utts[k]])
            assert fw.tolist() == rw.tolist()
            np.testing.assert_array_equal(fi["costs"], rc)
            assert on.frames[k] == 0
            utts[k], pos[k], reused = rng.normal(size=(9, 3)), 0, True
    assert reused and all(pos[k] == len(utts[k]) for k in range(5))
    on.reset()
    assert on.frames.tolist() == [0] * 5
    on.close()


def test_online_recognizer_refuses_before_the_backend_is_touched(fake_backend):
    from sr.recognition import _hip
    rng = np.random.default_rng(22)
    rec = make_recognizer(rng)
    with pytest.raises(ValueError):
        rec.online(n_streams=0)
    on = rec.online(n_streams=3)
    x = rng.normal(size=(4, 3))
    on.push([2, 0], [x, x[:3]])
    before, calls = on.frames, FakeWordStreamSession.pushes
    assert before.tolist() == [3, 0, 4] and calls == 1
    for ids, chunks in (([1, 1], [x, x]),                                 # an id twice
                        ([0, 3], [x, x]), ([-1], [x]),                    # ids out of range
                        ([[0]], [x]), ([0.5], [x]),                       # not a flat sequence of indices
                        ([0], [rng.normal(size=(4, 4))]),                 # another feature dimension
                        ([0], [x[0]]),                                    # not a [t, D] array
                        ([0, 1], [x])):                                   # chunks and ids do not pair up
        with pytest.raises(ValueError):
            on.push(ids, chunks)
        assert on.frames.tolist() == before.tolist() and FakeWordStreamSession.pushes == calls
    b = _hip.Batch(rec.ctx, [rng.normal(size=(8, 3)), x])
    for ids, kw in (([1, 2], dict(first=[0, 2], count=[8, 3])), ([1, 2], dict(first=[-1, 0])), ([1, 2], dict(count=[9, 1])),
                    ([1, 2], dict(first=[0, 0], count=[-1, 2])), ([1, 2], dict(first=[0]))):     # outside the utterance
        with pytest.raises(ValueError):
            on.push_batch(ids, b, **kw)
        assert on.frames.tolist() == before.tolist() and FakeWordStreamSession.pushes == calls
    with pytest.raises(ValueError):
        on.push_batch([1, 1], b)
    with pytest.raises(ValueError):
        on.push_batch([1], b)                                             # two utterances for one id
    with pytest.raises(ValueError):
        on.push_batch([1, 2], _hip.Batch(rec.ctx, [rng.normal(size=(8, 5)), rng.normal(size=(2, 5))]))
    with pytest.raises(ValueError):
        on.result([5])
    with pytest.raises(ValueError):
        on.reset([3])
    with pytest.raises(ValueError):
        on.finish([-1])
    assert on.frames.tolist() == before.tolist() and FakeWordStreamSession.pushes == calls
    on.push_batch([1, 2], b, first=[2, 0], count=[6, 4])
    assert on.frames.tolist() == [3, 6, 8]                                # (no capacity: streams take any number of frames)
    on.push([0], [np.zeros((0, 3))])                                      # an empty tick never reaches the backend
    on.push_batch([0, 1], b, count=[0, 0])
    on.push([], [])
    assert FakeWordStreamSession.pushes == calls + 1 and on.frames.tolist() == [3, 6, 8]
    # finish frees the ids: they start at frame 0 again, the others stay
    on.finish([1, 2])
    assert on.frames.tolist() == [3, 0, 0]
    on.push([1], [x])
    w1, i1 = on.result([1])
    rw, rc = rec.recognize([x])
    assert w1.tolist() == rw.tolist()
    np.testing.assert_array_equal(i1["costs"], rc)


def test_single_gaussian_recognisers_and_missing_objects_are_refused(fake_backend):
    from sr.recognition import _hip
    rng = np.random.default_rng(23)
    single = make_recognizer(rng, use_gmm=False)
    assert single.single
    with pytest.raises(_hip.Unsupported):
        single.online(n_streams=2)
    assert FakeWordStreamSession.pushes == 0
    on = make_recognizer(rng).online(n_streams=2)
    with pytest.raises(ValueError):
        on.push_audio([0], [np.zeros(400, dtype=np.int16)])               # no front-end
    with pytest.raises(ValueError):
        on.push_recording([0], [np.zeros(400, dtype=np.int16)])           # no endpointer
    assert on.frames.tolist() == [0, 0] and FakeWordStreamSession.pushes == 0


def test_push_audio_and_push_recording_on_the_doubles(fake_backend):
    from sr.audio_capture import StreamingEndpointer
    from sr.feature import StreamingFrontend
    from test_stream_endpoints_host import offline_ranges
    rng = np.random.default_rng(24)
    rec = make_recognizer(rng, D=39)
    # the compatibility checks of OnlineDecoder.__init__
    raw = dict(A.DEFAULT_CONFIG, **{'sample rate': 16000, 'silence threshold': 100, 'speech threshold': 50, 'start boundary': 20})
    cfg = A.derive(raw)
    ep = StreamingEndpointer(2, dict(raw), max_chunk=1600)
    for kw in (dict(frontend=StreamingFrontend(3)), dict(frontend=StreamingFrontend(2, dtype=np.float32)), dict(endpointer=ep),
               dict(frontend=StreamingFrontend(2, max_chunk=ep.max_piece - 1), endpointer=ep),
               dict(frontend=StreamingFrontend(2, 8000, max_chunk=4000), endpointer=ep),
               dict(frontend=StreamingFrontend(2, max_chunk=4000), endpointer=StreamingEndpointer(3, dict(raw))),
               dict(frontend=StreamingFrontend(2, max_chunk=40000),                  # utterances of 80 samples: fewer than 2 frames
                    endpointer=StreamingEndpointer(2, dict(raw, **{'frame time': 0.005, 'frame stride': 0.005, 'start boundary': 0})))):
        with pytest.raises(ValueError):
            rec.online(2, **kw)
    # audio: the result is recognize() of the whole utterance's features; a refused push moves neither object
    fe = StreamingFrontend(2, max_chunk=4000)
    on = rec.online(2, frontend=fe)
    sig = rng.integers(-3000, 3000, size=1700).astype(np.int16)
    on.push_audio([1], [sig[:1000]])
    state = (fe.samples.tolist(), on.frames.tolist(), FakeWordStreamSession.pushes, FakeStreamFrontend.pushes)
    for ids, chunks in (([1, 1], [sig[:10], sig[:10]]), ([2], [sig[:10]]), ([1], [sig[:10].astype(np.int32)])):
        with pytest.raises(ValueError):
            on.push_audio(ids, chunks)
        assert (fe.samples.tolist(), on.frames.tolist(), FakeWordStreamSession.pushes, FakeStreamFrontend.pushes) == state
    on.push_audio([1], [sig[1000:]], end=[True])
    words, info = on.finish([1])
    rw, rc = rec.recognize([raw_stack(O.mfcc_features_signal(sig, 16000)[1])])
    assert words.tolist() == rw.tolist()
    np.testing.assert_array_equal(info["costs"], rc)
    assert on.frames.tolist() == [0, 0] and fe.samples.tolist() == [0, 0]
    # recordings: the gate's (begin, stop, open) come back unchanged, the word is recognize() of that slice alone
    fe = StreamingFrontend(2, max_chunk=ep.max_piece)
    on = rec.online(2, frontend=fe, endpointer=ep)
    x = S.burst_signal(rng, 16000, 40, [(3000, 6000), (10000, 13000)], rate=16000)
    want, ref = offline_ranges(x, cfg)
    assert len(want) == 2 and not ref["open"]
    got = []
    for t in range(0, 16000, 1600):
        got += on.push_recording([1], [x[t:t + 1600]], [t + 1600 >= 16000])
    assert [sorted(u) for u in got] == [["begin", "costs", "open", "stop", "stream", "word"]] * 2
    assert [(u["stream"], u["begin"], u["stop"], u["open"]) for u in got] == [(1, b, e, False) for b, e in want]
    for u in got:
        rw, rc = rec.recognize([raw_stack(O.mfcc_features_signal(x[u["begin"]:u["stop"]], 16000)[1])])
        assert u["word"] == int(rw[0])
        np.testing.assert_array_equal(u["costs"], rc[0])
    assert on.frames.tolist() == [0, 0] and fe.samples.tolist() == [0, 0] and ep.samples.tolist() == [0, 16000]
    state = (ep.samples.tolist(), fe.samples.tolist(), on.frames.tolist(), S.FakeEndpointStream.pushes)
    for ids, chunks in (([0, 0], [x[:10], x[:10]]), ([1], [x[:10]]), ([0], [x[:1601]]), ([2], [x[:10]])):
        with pytest.raises(ValueError):
            on.push_recording(ids, chunks)
        assert (ep.samples.tolist(), fe.samples.tolist(), on.frames.tolist(), S.FakeEndpointStream.pushes) == state
    on.reset()                                                            # with an endpointer: a new recording
    assert ep.samples.tolist() == [0, 0]
