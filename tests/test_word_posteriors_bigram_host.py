# -*- coding: utf-8 -*-
"""Word posteriors and per-word confidence of the bigram grammar, on the host (no GPU).

1. The formula (tests/word_posteriors_bigram_ref.py: q from `O.forward_backward`) against brute-force enumeration of every
   path at 2 x 2, 3 x 2 (35 % of B at +inf, init[0] = +inf), 2 x 3 and 3 x 3 with skip arcs (one of them sparse), and with
   no path (3 x 3, T = 2; 2 x 3, T = 1): agreement, rows summing to one, and a column sum of gamma above 1.05 somewhere,
   all at 1e-12.  The per-column `sweep` and the np.longdouble recursion are held to the same formula.
2. A constant B = p with initial = 0 is the loop grammar with word_penalty = p.
3. A word that follows itself with certainty: confidences <= 1 where the per-word sum of gamma exceeds 1.5.
4. gh_word_posteriors_bigram is in the header, in the ctypes table and exported.
5. `ContinuousDecoder(grammar="bigram")` is refused without lm=True as it always was; with lm=True layers, a beam and 12
   states keep their own sentences and a loop decoder reaches `word_posteriors` -- on test doubles, nothing launched."""
import ctypes
import os
import re

import numpy as np
import pytest

import fake_hip
from conftest import ROOT
from oracle import ref_numpy as O
from word_posteriors_ref import word_posteriors as loop_word_posteriors
from word_posteriors_bigram_ref import (bigram_graph, brute_force, confidence, forward_backward, sweep, word_posteriors_bigram)
from test_word_posteriors_host import CountingBatch, UntouchedLattices, make_models, word_trans

TOL = 1e-12
#         W  n  T  skip   forbidden  init0_inf
CASES = [(2, 2, 5, False, 0.0, False),
         (3, 2, 5, False, 0.35, True),
         (2, 3, 6, True, 0.0, False),
         (3, 3, 6, True, 0.35, False),
         (3, 3, 2, False, 0.0, False),                                     # no path: T < n without skip arcs
         (2, 3, 1, False, 0.0, False)]                                     # no path: T = 1
CASE_IDS = ["%dx%d-T%d%s%s" % (c[0], c[1], c[2], "-skip" if c[3] else "", "-sparse" if c[4] else "") for c in CASES]


def bigram_case(W, n, T, skip, forbidden, init0_inf, seed=0):
    rng = np.random.default_rng(2600 + 1000 * W + 100 * n + 10 * T + skip + seed)
    wt = [word_trans(rng, n, skip) for _ in range(W)]
    for t in wt:                                                          # costs in [0, 3]
        t[~np.isinf(t)] = rng.uniform(0.0, 3.0, size=int((~np.isinf(t)).sum()))
    B = rng.uniform(0.0, 3.0, size=(W, W))
    if forbidden:
        B[rng.random((W, W)) < forbidden] = np.inf
        B[W - 1, 0] = 1.0                                                 # (at least one pair is left)
    init = rng.uniform(0.0, 3.0, size=W)
    if init0_inf:
        init[0] = np.inf
    trans, nes, rw, ends, entry, row_of = bigram_graph(wt, n, B, init)
    E = np.where(nes[:, None], 0.0, rng.uniform(0.5, 4.0, size=(len(nes), T)))
    return dict(W=W, n=n, T=T, wt=wt, B=B, init=init, trans=trans, nes=nes, rw=rw, ends=ends, entry=entry, row_of=row_of, E=E)


def states_of(c):
    """Es [T, W, n] of the per-column sweep from the [R, T] emissions of the graph."""
    return np.transpose(c["E"][c["row_of"]], (2, 0, 1))


@pytest.mark.parametrize("shape", CASES, ids=CASE_IDS)
def test_formula_equals_brute_force(shape):
    c = bigram_case(*shape)
    post, logp = word_posteriors_bigram(c["E"], c["nes"], c["rw"], c["trans"], c["ends"], c["entry"], c["row_of"])
    bf, bf_logp = brute_force(c["E"], c["nes"], c["rw"], c["trans"], c["ends"], c["W"])
    no_path = c["T"] < c["n"]
    if no_path:
        assert logp == -np.inf and bf_logp == -np.inf and not post.any() and not bf.any()
        np.testing.assert_array_equal(confidence(post, [1], [0], c["T"]), [0.0])
    else:
        assert np.isfinite(logp)
        np.testing.assert_allclose(logp, bf_logp, rtol=TOL, atol=TOL)
        print("max |q - enumeration| = %.3g, max |row sum - 1| = %.3g" % (np.max(np.abs(post - bf)), np.max(np.abs(post.sum(axis=1) - 1))))
        np.testing.assert_allclose(post, bf, rtol=0, atol=TOL)
        np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=TOL)
        assert post.min() >= 0.0 and post.max() <= 1.0 + TOL
    # the per-column sweep and the extended-precision recursion state the same thing
    sp, slogp, gsum = sweep(c["wt"], c["B"], c["init"], states_of(c))
    lp, llogp = word_posteriors_bigram(c["E"], c["nes"], c["rw"], c["trans"], c["ends"], c["entry"], c["row_of"], dtype=np.longdouble)
    xp, xlogp, _ = sweep(c["wt"], c["B"], c["init"], states_of(c), dtype=np.longdouble)
    assert lp.dtype == np.longdouble and xp.dtype == np.longdouble
    for other, other_logp in ((sp, slogp), (lp, llogp), (xp, xlogp)):
        if no_path:
            assert other_logp == -np.inf and not other.any()
        else:
            np.testing.assert_allclose(float(other_logp), logp, rtol=TOL, atol=TOL)
            np.testing.assert_allclose(np.asarray(other, dtype=np.float64), post, rtol=0, atol=TOL)


def test_the_correction_is_not_vacuous():
    """Summed over the words, gamma of a column exceeds 1 wherever a path crosses a word boundary in it."""
    most = 0.0
    for shape in CASES:
        c = bigram_case(*shape)
        gamma = O.forward_backward(c["E"], c["nes"], c["trans"], c["ends"])[2]
        most = max(most, float(gamma[~c["nes"]].sum(axis=0).max()))
        gsum = sweep(c["wt"], c["B"], c["init"], states_of(c))[2]
        np.testing.assert_allclose(gsum.sum(axis=1), gamma[~c["nes"]].sum(axis=0), rtol=0, atol=TOL)
    print("largest column sum of gamma: %.3f" % most)
    assert most > 1.05


def test_the_sweep_equals_the_formula_on_a_wide_sparse_graph():
    """17 words x 3 states with skip arcs, 35 % of the pairs forbidden: the size class the GPU tests restate with `sweep`."""
    c = bigram_case(17, 3, 12, True, 0.35, True, seed=1)
    post, logp = word_posteriors_bigram(c["E"], c["nes"], c["rw"], c["trans"], c["ends"], c["entry"], c["row_of"])
    sp, slogp, _ = sweep(c["wt"], c["B"], c["init"], states_of(c))
    assert np.isfinite(logp)
    np.testing.assert_allclose(slogp, logp, rtol=TOL)
    np.testing.assert_allclose(sp, post, rtol=0, atol=TOL)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=TOL)


@pytest.mark.parametrize("W,n,skip,T,p", [(2, 2, False, 6, 0.7), (3, 3, True, 9, 0.0), (4, 4, False, 11, 2.5)])
def test_constant_costs_are_the_loop_grammar(W, n, skip, T, p):
    rng = np.random.default_rng(31 + W + n)
    wt = [word_trans(rng, n, skip) for _ in range(W)]
    trans, nes, rw, ends, entry, row_of = bigram_graph(wt, n, np.full((W, W), p), np.zeros(W))
    lnes, lrw, lrs, ldense, lends = O.loop_grammar(wt, n, p)
    Es = rng.uniform(0.2, 4.0, size=(T, W, n))
    E = np.zeros((len(nes), T))
    E[row_of] = np.transpose(Es, (1, 2, 0))
    lE = np.zeros((len(lnes), T))
    for w in range(W):
        for s in range(n):
            lE[np.flatnonzero((lrw == w) & (lrs == s))[0]] = Es[:, w, s]
    post, logp = word_posteriors_bigram(E, nes, rw, trans, ends, entry, row_of)
    lpost, llogp = loop_word_posteriors(lE, lnes, lrw, ldense, lends, W, n)
    assert np.isfinite(logp)
    np.testing.assert_allclose(logp, llogp, rtol=TOL)
    np.testing.assert_allclose(post, lpost, rtol=0, atol=TOL)


def test_a_word_that_follows_itself_keeps_its_confidences_below_one():
    """Two words; word 0 can only be followed by itself, and the emissions pull the path through it twice: the boundary
    frame is occupied by both passes (per-word gamma sum near 2), the posterior of word 0 stays 1."""
    W, n, T = 2, 3, 9
    rng = np.random.default_rng(5)
    wt = [word_trans(rng, n, False) for _ in range(W)]
    B = np.array([[0.2, np.inf], [np.inf, np.inf]])
    trans, nes, rw, ends, entry, row_of = bigram_graph(wt, n, B, np.array([0.1, np.inf]))
    E = np.full((len(nes), T), 6.0)
    E[nes] = 0.0
    for t, s in enumerate([0, 0, 1, 2, 2, 0, 1, 1, 2]):
        E[row_of[0, s], t] = 0.1
    E[row_of[0, 0], 4] = 0.1                                              # frame 4: last state of pass one, first of pass two
    costs, path = O.decode_states(E, nes, trans, end_points=[[int(e), -1] for e in ends])
    cells = np.asarray(path)[::-1]
    emitting = ~nes[cells[:, 0]]
    first = emitting & np.insert(~emitting[:-1], 0, True)
    words, begins = [int(w) for w in rw[cells[first, 0]]], [int(b) for b in cells[first, 1]]
    assert words == [0, 0] and begins[0] == 0 and 0 < begins[1] < T
    post, logp = word_posteriors_bigram(E, nes, rw, trans, ends, entry, row_of)
    gamma = O.forward_backward(E, nes, trans, ends)[2]
    per_word = gamma[rw == 0].sum(axis=0)
    assert per_word[begins[1]] > 1.5
    conf = confidence(post, words, begins, T)
    assert conf.shape == (2,) and np.all(conf <= 1.0 + TOL) and np.all(conf > 0.99)
    np.testing.assert_allclose(post[:, 0], 1.0, rtol=0, atol=TOL)
    assert not post[:, 1].any()


def test_the_extended_precision_recursion_is_the_oracles():
    c = bigram_case(3, 3, 6, True, 0.35, False)
    la, lb, gamma, logp = O.forward_backward(c["E"], c["nes"], c["trans"], c["ends"])
    xa, xb, xg, xlogp = forward_backward(c["E"], c["nes"], c["trans"], c["ends"], dtype=np.longdouble)
    assert xa.dtype == np.longdouble
    fin = np.isfinite(la)
    np.testing.assert_array_equal(np.isfinite(xa), fin)
    np.testing.assert_allclose(np.asarray(xa[fin], dtype=np.float64), la[fin], rtol=TOL)
    fin = np.isfinite(lb)
    np.testing.assert_array_equal(np.isfinite(xb), fin)
    np.testing.assert_allclose(np.asarray(xb[fin], dtype=np.float64), lb[fin], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(float(xlogp), logp, rtol=TOL)


def test_header_binding_and_library_have_the_entry(built_library):
    from sr.recognition import _hip
    raw = open(os.path.join(ROOT, "include", "gmmhmm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+gh_word_posteriors_bigram\s*\(", text)
    assert "NOT in the reference" in raw[raw.index("word posteriors and per-word confidence (bigram form)"):raw.index("int gh_word_posteriors_bigram")]
    assert "gh_word_posteriors_bigram" in _hip.SIGNATURES
    assert _hip.SIGNATURES["gh_word_posteriors_bigram"] == _hip.SIGNATURES["gh_word_posteriors"]
    res, args = _hip.SIGNATURES["gh_word_posteriors_bigram"]
    assert res is ctypes.c_int and len(args) == 10
    assert hasattr(ctypes.CDLL(built_library), "gh_word_posteriors_bigram")
    assert callable(getattr(_hip.Lattices, "word_posteriors_bigram"))


# ----------------------------------------------------------------------------------------------------------------------
class RecordingLattices(fake_hip.Lattices):
    """Test double of `_hip.Lattices` that answers the timed label decode through the oracle and records which posterior
    method the decoder reaches (neither computes anything here)."""
    reached = []

    def forms(self):
        return set()

    def viterbi_labels(self, batch, row_label, max_labels=None, want_begin=False, **kw):
        from sr.recognition.batch import path_to_word_times
        r = self.viterbi(batch, want_path=True)
        rs, n = np.asarray(self.graphs[0]["row_state"]), int(np.asarray(row_label).tolist().count(0))
        wt = [path_to_word_times(p, rs, n) for p in r["paths"]]
        out = dict(labels=[np.array(w, dtype=np.int32) for w, _ in wt], best_end=r["best_end"], end_cost_flat=r["end_cost_flat"])
        if want_begin:
            out["begins"] = [np.array(b, dtype=np.int32) for _, b in wt]
        return out

    def word_posteriors(self, batch, labels=None, begins=None, want_post=True):
        type(self).reached.append("word_posteriors")
        return dict(logp=np.zeros(batch.U), post=np.zeros((batch.N, 1)), confidence=[np.zeros(len(l)) for l in (labels or [])])

    def word_posteriors_bigram(self, batch, labels=None, begins=None, want_post=True):
        type(self).reached.append("word_posteriors_bigram")
        return dict(logp=np.zeros(batch.U), post=np.zeros((batch.N, 1)), confidence=[np.zeros(len(l)) for l in (labels or [])])


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "Lattices", UntouchedLattices)
    monkeypatch.setattr(_hip, "Batch", CountingBatch)
    monkeypatch.setattr(UntouchedLattices, "calls", 0)
    monkeypatch.setattr(CountingBatch, "made", 0)
    monkeypatch.setattr(CountingBatch, "scored", 0)
    monkeypatch.setattr(RecordingLattices, "reached", [])
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield monkeypatch
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def test_without_the_keyword_a_bigram_decoder_is_refused_as_before(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(11)
    hmms = make_models(rng, 3, 3)
    xs = [rng.normal(size=(12, 3)), rng.normal(size=(9, 3))]
    dec = ContinuousDecoder(hmms, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3)))
    b = _hip.Batch(dec.ctx, xs)
    made = CountingBatch.made
    for call in (lambda: dec.decode_batch(b, want_confidence=True), lambda: dec.word_posteriors(b),
                 lambda: dec.decode(xs, want_confidence=True),
                 lambda: dec.decode_batch(b, want_confidence=True, lm=False), lambda: dec.word_posteriors(b, lm=False),
                 lambda: dec.decode(xs, want_confidence=True, lm=False)):
        with pytest.raises(_hip.Unsupported, match="bigram grammar"):
            call()
    assert CountingBatch.made == made and CountingBatch.scored == 0 and UntouchedLattices.calls == 0


def test_with_the_keyword_the_other_refusals_keep_their_sentences(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(12)
    hmms = make_models(rng, 3, 3)
    xs = [rng.normal(size=(12, 3)), rng.normal(size=(9, 3))]
    beamed = ContinuousDecoder(hmms, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3)))
    beamed.lat.set_beam(4)
    cases = [(ContinuousDecoder(hmms, n_layers=2), "K-layer lattice"),
             (beamed, "rank beam"),
             (ContinuousDecoder(make_models(rng, 2, 12), grammar="bigram", bigram=np.ones((2, 2))), "2 to 8 states, not 12")]
    sentences = set()
    for dec, hint in cases:
        b = _hip.Batch(dec.ctx, xs)
        made = CountingBatch.made
        for call in (lambda: dec.decode_batch(b, want_confidence=True, lm=True), lambda: dec.word_posteriors(b, lm=True),
                     lambda: dec.decode(xs, want_confidence=True, lm=True)):
            with pytest.raises(_hip.Unsupported, match=hint) as e:
                call()
            sentences.add(str(e.value))
        assert CountingBatch.made == made and CountingBatch.scored == 0 and UntouchedLattices.calls == 0
    assert len(sentences) == len(cases)
    dec = ContinuousDecoder(hmms, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3)))
    with pytest.raises(ValueError):
        dec.decode_batch(_hip.Batch(dec.ctx, xs), want_path=True, want_confidence=True, lm=True)
    assert UntouchedLattices.calls == 0
    # the online decoders do not take the keyword
    import inspect
    from sr.recognition import batch as B
    for name in ("OnlineDecoder", "OnlineBigramDecoder", "OnlineLayersDecoder"):
        for meth in ("result", "commit", "tail", "finish", "push", "__init__"):
            fn = getattr(getattr(B, name), meth, None)
            if fn is not None:
                assert "lm" not in inspect.signature(fn).parameters


def test_the_keyword_routes_by_grammar(fake_backend):
    """lm=True on a loop decoder reaches `word_posteriors`, on a bigram decoder `word_posteriors_bigram`; without
    want_confidence it changes nothing."""
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    fake_backend.setattr(_hip, "Lattices", RecordingLattices)
    rng = np.random.default_rng(13)
    hmms = make_models(rng, 3, 3)
    xs = [rng.normal(size=(12, 3)), rng.normal(size=(9, 3))]
    loop = ContinuousDecoder(hmms, grammar="loop")
    bigram = ContinuousDecoder(hmms, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3)))
    for dec, want in ((loop, "word_posteriors"), (bigram, "word_posteriors_bigram")):
        del RecordingLattices.reached[:]
        b = _hip.Batch(dec.ctx, xs)
        words, r = dec.decode_batch(b, want_confidence=True, lm=True)
        timed_words, timed = dec.decode_batch(b, want_times=True)
        assert words == timed_words and "confidence" in r and "logp" in r and "confidence" not in timed
        for u in range(len(xs)):
            np.testing.assert_array_equal(r["begins"][u], timed["begins"][u])
        dec.word_posteriors(b, lm=True)
        w3, b3, c3 = dec.decode(xs, want_confidence=True, lm=True)
        assert w3 == words and RecordingLattices.reached == [want] * 3
        del RecordingLattices.reached[:]
        plain_words, plain = dec.decode_batch(b, lm=True)
        assert plain_words == dec.decode_batch(b)[0] == dec.decode(xs, lm=True) and "confidence" not in plain
        assert dec.decode(xs, want_times=True, lm=True)[0] == words
        assert RecordingLattices.reached == []
