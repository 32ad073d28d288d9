# -*- coding: utf-8 -*-
"""Forward scores, vocabulary posteriors and rejection for the isolated-word recogniser, on the host (no GPU).

1. The vectorised restatement (tests/word_forward_ref.py) == `O.forward_backward` per chain: log P to 1e-12, the same -inf
   cells, n = 1 .. 8 with and without skip arcs, T in {1, 2, n-1, n, 12}.
2. `O.forward_backward` == brute-force enumeration of every path at 3 states x 5 frames and 4 states with skip arcs x 5.
3. soft <= the oracle's Viterbi end cost everywhere, and == it exactly where exactly one path exists (T == n, no skip arcs).
   (T = 1 is compared against the causal column 0, `CarriedDecode`: the oracle's one-frame decode is the reference's column
   wrap, which the recogniser does not reproduce -- tests/test_online_words_host.py.)
4. The softmax: rows sum to 1, scale -> 0+ tends to the prior, a -inf prior zeroes its word, an all-+inf row is a zero row.
5. `min_confidence`, the info dict and the refusals on doubles of the backend, with nothing launched by a refused call.
6. The three new entry points are in the header, in the ctypes table and exported by the built library."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import fake_hip
import word_forward_ref as F
from online_ref import CarriedDecode
from oracle import ref_numpy as O
from word_posteriors_ref import brute_force

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lengths(n):
    return sorted({T for T in (1, 2, n - 1, n, 12) if T >= 1})


# ------------------------------------------------------------------------------------------------ 1: the restatement
@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("n", range(1, 9))
def test_restatement_is_the_oracle_per_chain(n, skip):
    rng = np.random.default_rng(10 * n + skip)
    W = 3
    trans = [F.word_trans(rng, n, skip) for _ in range(W)]
    c = F.chain_costs(trans)
    seen_inf = False
    for T in lengths(n):
        E = rng.uniform(0.5, 9.0, size=(W, n, T))
        if T == 12:
            E[1, n // 2, 5] = np.inf                                     # an emission that underflowed
        al = F.forward_alpha(E, *c)
        soft = F.soft_costs(E, *c)
        for w in range(W):
            la, _, _, logp = O.forward_backward(E[w], np.zeros(n, dtype=bool), trans[w], [n - 1])
            np.testing.assert_array_equal(np.isneginf(al[w]), np.isneginf(la))
            fin = np.isfinite(la)
            np.testing.assert_allclose(al[w][fin], la[fin], rtol=1e-12)
            if np.isneginf(logp):
                assert soft[w] == np.inf
                seen_inf = True
            else:
                np.testing.assert_allclose(-soft[w], logp, rtol=1e-12)
        if T < n and not skip:
            assert np.all(np.isposinf(soft))                             # fewer frames than states, no skip arcs: no path
    assert seen_inf
    assert np.all(np.isposinf(F.soft_costs(np.zeros((W, n, 0)), *c)))    # no frames


# ------------------------------------------------------------------------------------------------ 2: the oracle itself
@pytest.mark.parametrize("n,skip", [(3, False), (4, True)])
def test_oracle_is_the_sum_over_every_path(n, skip):
    rng = np.random.default_rng(n)
    trans = F.word_trans(rng, n, skip)
    E = rng.uniform(0.5, 4.0, size=(n, 5))
    nes = np.zeros(n, dtype=bool)
    _, logp_bf = brute_force(E, nes, np.zeros(n, dtype=int), trans, [n - 1], 1)
    _, _, _, logp = O.forward_backward(E, nes, trans, [n - 1])
    assert np.isfinite(logp)
    np.testing.assert_allclose(logp, logp_bf, rtol=1e-12)
    np.testing.assert_allclose(-F.soft_costs(E[None], *F.chain_costs([trans]))[0], logp_bf, rtol=1e-12)


# ------------------------------------------------------------------------------------------------ 3: against Viterbi
def viterbi_end_cost(E, trans):
    n, T = E.shape
    if T == 1:                                                           # the causal column 0 (see the module docstring)
        cd = CarriedDecode(np.zeros(n, dtype=bool), trans, [n - 1])
        cd.push(E)
        return cd.result()[0][0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        costs, _ = O.decode_fill(E, np.zeros(n, dtype=bool), trans)
    return costs[n - 1, T - 1]


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("n", range(1, 9))
def test_soft_cost_is_below_the_viterbi_cost_and_equal_on_one_path(n, skip):
    rng = np.random.default_rng(50 + 10 * n + skip)
    trans = F.word_trans(rng, n, skip)
    c = F.chain_costs([trans])
    for T in lengths(n):
        E = rng.uniform(0.5, 9.0, size=(n, T))
        soft = F.soft_costs(E[None], *c)[0]
        cost = viterbi_end_cost(E, trans)
        assert np.isposinf(soft) == np.isposinf(cost)
        assert soft <= cost
        if T == n and not skip:
            assert soft == cost                                          # exactly one path: the sum has one term
        elif np.isfinite(cost) and T > n >= 2:
            assert soft < cost                                           # several paths
        elif n == 1:
            assert soft == cost                                          # a one-state word has one path at every length


# ------------------------------------------------------------------------------------------------ 4: the softmax
def test_softmax_over_the_vocabulary():
    rng = np.random.default_rng(4)
    U, W = 9, 6
    soft = rng.uniform(200.0, 260.0, size=(U, W))
    soft[2, 3] = np.inf                                                  # a word without a path
    soft[5] = np.inf                                                     # an utterance no word has a path for
    post = F.vocabulary_posteriors(soft)
    live = np.arange(U) != 5
    np.testing.assert_allclose(post[live].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert post[2, 3] == 0.0 and not post[5].any() and np.all(post >= 0.0)
    np.testing.assert_array_equal(np.argmax(post[live], axis=1), np.argmin(soft[live], axis=1))
    # by the definition, written out
    z = soft[0]
    p = np.exp(z.min() - z)
    s = 0.0
    for v in p:
        s = s + v
    np.testing.assert_array_equal(post[0], p / s)
    # scale flattens; scale -> 0+ tends to the prior
    lp = np.log(rng.dirichlet(np.ones(W)))
    flat = F.vocabulary_posteriors(soft, scale=0.05)
    assert np.all(flat[live].max(axis=1) < post[live].max(axis=1))
    tiny = F.vocabulary_posteriors(soft[:2], scale=1e-12, log_prior=lp)
    np.testing.assert_allclose(tiny, np.tile(np.exp(lp), (2, 1)), rtol=1e-8)
    # a -inf prior zeroes its word, the others share the mass
    lp2 = np.zeros(W)
    lp2[1] = -np.inf
    off = F.vocabulary_posteriors(soft, log_prior=lp2)
    assert not off[:, 1].any()
    np.testing.assert_allclose(off[live].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    only = np.full((1, W), np.inf)
    only[0, 1] = 3.0
    assert not F.vocabulary_posteriors(only, log_prior=lp2).any()      # its one path is a forbidden word
    assert F.vocabulary_posteriors(np.zeros((0, W))).shape == (0, W)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            F.vocabulary_posteriors(soft, scale=bad)
    for bad in (np.zeros(W - 1), np.zeros((1, W)), np.full(W, np.nan), np.full(W, np.inf)):
        with pytest.raises(ValueError):
            F.vocabulary_posteriors(soft, log_prior=bad)


def test_zero_row_has_no_soft_word_and_no_confidence():
    from sr.recognition.batch import _posterior_info
    soft = np.array([[3.0, 2.0, 2.0], [np.inf, np.inf, np.inf], [1.0, np.inf, 4.0]])
    info = _posterior_info(soft, np.array([1, 0, -1]), 1.0, None)
    assert set(info) == {"soft_costs", "posteriors", "confidence", "soft_words"}
    assert info["soft_words"].tolist() == [1, -1, 0]                     # the FIRST arg-max; -1 for the zero row
    assert info["confidence"][1] == 0.0 and info["confidence"][2] == 0.0
    assert info["confidence"][0] == info["posteriors"][0, 1]
    assert info["soft_costs"] is soft


# ------------------------------------------------------------------------------------------------ 5: host logic on doubles
class Touch:
    """Counts what reaches the doubles of the backend."""
    n = 0


class SoftLattices(fake_hip.Lattices):
    def chain_forward(self, batch):
        Touch.n += 1
        g = self.graphs[0]
        dense = self._dense(g)
        starts = sorted(int(s) for s in g["start_rows"])
        n = starts[1] - starts[0] if len(starts) > 1 else len(g["row_state"])
        trans = [dense[s:s + n, s:s + n] for s in starts]
        return F.soft_costs_batch(batch.nll, batch.offsets, trans)


class SoftBatch(fake_hip.Batch):
    def __init__(self, *a, **kw):
        Touch.n += 1
        super().__init__(*a, **kw)


class SoftSession:
    """Double of `_hip.WordStreamSession(soft=True)`: keeps every stream's likelihood rows and scores the prefix anew."""

    def __init__(self, ctx, lat, n_streams, soft=False):
        Touch.n += 1
        self.lat, self.n_streams, self.soft = lat, int(n_streams), soft
        self.rows = [np.zeros((0, len(lat.graphs[0]["row_state"]))) for _ in range(self.n_streams)]
        self.n_end = lat.n_end[0]

    def push(self, batch, ids, first=None, count=None):
        Touch.n += 1
        first = np.zeros(batch.U, dtype=np.int64) if first is None else np.asarray(first)
        count = batch.lengths - first if count is None else np.asarray(count)
        for u, k in enumerate(ids):
            lo = batch.offsets[u] + first[u]
            self.rows[int(k)] = np.concatenate([self.rows[int(k)], batch.nll[lo:lo + count[u]]])

    def reset(self, ids=None):
        for k in (range(self.n_streams) if ids is None else ids):
            self.rows[int(k)] = self.rows[int(k)][:0]

    def _batch(self, ids):
        b = fake_hip.Batch(None, [np.zeros((len(self.rows[int(k)]), 1)) for k in ids])
        b.nll = np.concatenate([self.rows[int(k)] for k in ids])
        b.S = b.nll.shape[1]
        return b

    def result(self, ids):
        b = self._batch(ids)
        costs = self.lat.viterbi(b, want_path=False)["end_cost_flat"].reshape(len(ids), self.n_end)
        T = b.lengths
        return dict(costs=costs, best=np.where(T > 0, np.argmin(costs, axis=1), -1).astype(np.int32), frames=T)

    def result_soft(self, ids):
        assert self.soft
        Touch.n -= 1                                                     # (the double's own use of chain_forward)
        return self.lat.chain_forward(self._batch(ids))

    def close(self):
        pass


@pytest.fixture
def doubles(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "Lattices", SoftLattices)
    monkeypatch.setattr(_hip, "Batch", SoftBatch)
    monkeypatch.setattr(_hip, "WordStreamSession", SoftSession, raising=False)
    monkeypatch.setattr(Touch, "n", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


W_, N_, D_ = 4, 3, 3


def make_recognizer(rng, M=2, use_gmm=True):
    import sr.recognition as R
    from sr.recognition.batch import IsolatedWordRecognizer
    hmms = []
    for i in range(W_):
        h = R.HMM(N_)
        mean, var = rng.normal(size=(N_, M, D_)) * 3.0, rng.uniform(0.5, 1.5, size=(N_, M, D_))
        h.mu, h.sigma = mean[:, 0].copy(), var[:, 0].copy()
        h.use_gmm = use_gmm
        h.gmm_states = None
        if use_gmm:
            h.gmm_states = []
            for s in range(N_):
                g = R.GMM(mean[s, 0].copy(), var[s, 0].copy(), M)
                g.update_models(mean[s], var[s], rng.dirichlet(np.ones(M)))
                h.gmm_states.append(g)
        h.transitions = F.word_trans(rng, N_)
        hmms.append(h)
    return IsolatedWordRecognizer(hmms)


def test_recognize_with_posteriors_and_rejection(doubles):
    rng = np.random.default_rng(8)
    rec = make_recognizer(rng)
    xs = [rng.normal(size=(T, D_)) * 2.0 for T in (7, 2, 11, 5)]         # (2 frames: no word of 3 states has a path)
    plain = rec.recognize(xs)
    assert len(plain) == 2
    words, costs, info = rec.recognize(xs, want_posteriors=True)
    np.testing.assert_array_equal(words, plain[0])                       # the words stay the Viterbi arg-min
    np.testing.assert_array_equal(costs, plain[1])
    assert set(info) == {"soft_costs", "posteriors", "confidence", "soft_words"}
    assert info["soft_costs"].shape == (4, W_) and np.all(info["soft_costs"] <= costs)
    np.testing.assert_array_equal(info["posteriors"], F.vocabulary_posteriors(info["soft_costs"]))
    np.testing.assert_array_equal(info["confidence"], info["posteriors"][np.arange(4), words])
    assert np.all(np.isposinf(info["soft_costs"][1])) and info["confidence"][1] == 0.0 and info["soft_words"][1] == -1
    live = [0, 2, 3]
    np.testing.assert_allclose(info["posteriors"][live].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # rejection: below the threshold the word is -1, the costs and the info stay
    c = np.sort(info["confidence"])[2]
    w2, c2, i2 = rec.recognize(xs, want_posteriors=True, min_confidence=c)
    np.testing.assert_array_equal(w2, np.where(info["confidence"] < c, -1, words))
    assert (w2 == -1).sum() == 2
    np.testing.assert_array_equal(c2, costs)
    w3, _, _ = rec.recognize(xs, want_posteriors=True, min_confidence=1.5)
    assert w3.tolist() == [-1] * 4
    # scale and prior reach the softmax
    lp = np.log([0.7, 0.1, 0.1, 0.1])
    _, _, i4 = rec.recognize(xs, want_posteriors=True, scale=0.1, log_prior=lp)
    np.testing.assert_array_equal(i4["posteriors"], F.vocabulary_posteriors(info["soft_costs"], 0.1, lp))
    b = fake_hip.Batch(None, xs)
    post, soft = rec.posteriors(b, scale=0.1, log_prior=lp)
    np.testing.assert_array_equal(post, i4["posteriors"])
    np.testing.assert_array_equal(soft, rec.soft_costs(b))


def test_refusals_come_before_the_backend(doubles):
    from sr.recognition import _hip
    rng = np.random.default_rng(9)
    rec = make_recognizer(rng)
    xs = [rng.normal(size=(6, D_))]
    b = fake_hip.Batch(None, xs)
    Touch.n = 0
    with pytest.raises(ValueError, match="min_confidence needs want_posteriors"):
        rec.recognize(xs, min_confidence=0.5)
    for kw in (dict(scale=0.0), dict(scale=-2.0), dict(scale=np.inf), dict(scale=np.nan), dict(log_prior=np.zeros(W_ + 1)),
               dict(log_prior=np.full(W_, np.nan))):
        with pytest.raises(ValueError):
            rec.recognize(xs, want_posteriors=True, **kw)
        with pytest.raises(ValueError):
            rec.posteriors(b, **kw)
        with pytest.raises(ValueError):
            rec.online(2, soft=True, **kw)
    assert Touch.n == 0
    for single in (make_recognizer(rng, M=1), make_recognizer(rng, use_gmm=False)):   # one Gaussian per state: the fused sweep
        assert single.gmm.M == 1
        Touch.n = 0
        for call in (lambda: single.soft_costs(b), lambda: single.posteriors(b), lambda: single.recognize(xs, want_posteriors=True)):
            with pytest.raises(_hip.Unsupported, match="one Gaussian per state"):
                call()
        assert Touch.n == 0
        assert len(single.recognize(xs)) == 2                            # ... which goes on recognising
    with pytest.raises(_hip.Unsupported):
        make_recognizer(rng, use_gmm=False).online(2, soft=True)


def test_online_soft_reports_what_recognize_reports(doubles):
    rng = np.random.default_rng(10)
    rec = make_recognizer(rng)
    lp = np.log([0.4, 0.3, 0.2, 0.1])
    xs = [rng.normal(size=(T, D_)) * 2.0 for T in (9, 4)]
    plain = rec.online(3)
    plain.push([0, 1], xs)
    _, pinfo = plain.result([0, 1])
    assert set(pinfo) == {"costs", "frames"} and not plain.soft           # without soft=True everything is as before
    on = rec.online(3, soft=True, scale=0.5, log_prior=lp)
    on.push([2, 0], [x[:3] for x in xs])
    on.push([0, 2], [xs[1][3:], xs[0][3:]])
    words, info = on.result([2, 0, 1])
    rw, rc, ri = rec.recognize(xs, want_posteriors=True, scale=0.5, log_prior=lp)
    np.testing.assert_array_equal(words[:2], rw)
    for k in ("soft_costs", "posteriors", "confidence", "soft_words"):
        np.testing.assert_array_equal(info[k][:2], ri[k])
    assert words[2] == -1 and np.all(np.isposinf(info["soft_costs"][2])) and not info["posteriors"][2].any()
    assert info["confidence"][2] == 0.0 and info["soft_words"][2] == -1   # a stream without frames
    fw, fi = on.finish([2])
    np.testing.assert_array_equal(fi["confidence"], ri["confidence"][:1])
    assert on.frames[2] == 0


# ------------------------------------------------------------------------------------------------ 6: the entry points
def test_header_binding_and_library_have_the_entries(built_library):
    from sr.recognition import _hip
    raw = open(os.path.join(ROOT, "include", "gmmhmm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(built_library)
    for name, n_args in (("gh_chain_forward", 4), ("gh_wordstream_create_soft", 4), ("gh_wordstream_result_soft", 5)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        res, args = _hip.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args
        assert hasattr(lib, name)
    assert "NOT IN THE REFERENCE" in raw[raw.index("forward scores of word chains"):raw.index("int gh_chain_forward")]
    assert callable(_hip.Lattices.chain_forward) and callable(_hip.WordStreamSession.result_soft)
