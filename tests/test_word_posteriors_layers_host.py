# -*- coding: utf-8 -*-
"""Word posteriors on the K-layer lattice, on the host: the restatement (tests/word_posteriors_layers_ref.py) against
enumeration of every path, its properties, the mixture identity against the word loop, and the host logic of the `layers=`
keyword on test doubles.  No GPU; nothing is launched.

Bounds: 1e-12 absolute for posteriors against enumeration and for the identity -- a few hundred fp64 terms per cell, each
with a relative error of a few 1e-16 on values <= 1; measured 3.6e-15 and 6.3e-15."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import ref_numpy as O
from word_posteriors_ref import word_posteriors as loop_word_posteriors
from word_posteriors_layers_ref import (brute_force, emissions, forward_backward, layers_graph, q_from_matrices, sweep,
                                        word_posteriors_layers)
from test_word_posteriors_host import CountingBatch, UntouchedLattices, make_models, word_trans
from test_word_posteriors_bigram_host import RecordingLattices, fake_backend  # noqa: F401  (the fixture)

TOL = 1e-12


def layer_case(W, n, K, T, skip, seed=0):
    rng = np.random.default_rng(2700 + 1000 * K + 100 * W + 10 * n + skip + seed)
    wt = [word_trans(rng, n, skip) for _ in range(W)]
    costs = rng.uniform(0.5, 6.0, size=(T, W * n))
    rw, rs, nes, trans, ends = layers_graph(wt, n, K)
    return dict(W=W, n=n, K=K, T=T, wt=wt, costs=costs, rw=rw, rs=rs, nes=nes, trans=trans, ends=ends,
                E=emissions(costs, rw, rs, n))


def restate(c, dtype=np.float64):
    return word_posteriors_layers(c["E"], c["nes"], c["trans"], c["ends"], c["W"], c["n"], c["K"], dtype)


def swept(c, dtype=np.float64):
    return sweep(c["wt"], c["costs"].reshape(c["T"], c["W"], c["n"]), c["K"], dtype)


@pytest.mark.parametrize("shape", [(2, 2, 2, 4, False), (2, 2, 3, 5, False), (3, 2, 2, 4, False), (2, 3, 2, 5, True),
                                   (2, 3, 3, 6, True)], ids=lambda s: "W%d-n%d-K%d-T%d-%s" % (s[:4] + ("skip" if s[4] else "plain",)))
def test_formula_equals_brute_force(shape):
    c = layer_case(*shape)
    q, logp, qk = restate(c)
    bq, blogp = brute_force(c["E"], c["nes"], c["rw"], c["trans"], c["ends"], c["W"])
    print("max |q - enumeration|: %.3g" % np.abs(q - bq).max())
    assert np.isfinite(logp) and abs(logp - blogp) <= TOL * max(1.0, abs(blogp))
    np.testing.assert_allclose(q, bq, rtol=0, atol=TOL)
    np.testing.assert_allclose(q.sum(axis=1), 1.0, rtol=0, atol=TOL)
    assert q.min() >= 0.0 and q.max() <= 1.0 + TOL and qk.shape == (c["T"], c["K"], c["W"])
    for other in (restate(c, np.longdouble), swept(c), swept(c, np.longdouble)):
        np.testing.assert_allclose(np.asarray(other[0], dtype=np.float64), bq, rtol=0, atol=TOL)
        assert abs(float(other[1]) - blogp) <= TOL * max(1.0, abs(blogp))


@pytest.mark.parametrize("shape", [(2, 2, 2, 2, False), (2, 2, 3, 3, False), (2, 3, 2, 3, False), (2, 2, 2, 1, False),
                                   (3, 3, 1, 1, True)], ids=lambda s: "W%d-n%d-K%d-T%d" % s[:4])
def test_no_path_gives_minus_infinity_and_zero_rows(shape):
    c = layer_case(*shape)
    bq, blogp = brute_force(c["E"], c["nes"], c["rw"], c["trans"], c["ends"], c["W"])
    assert blogp == -np.inf and not bq.any()
    for q, logp in (restate(c)[:2], restate(c, np.longdouble)[:2], swept(c)[:2]):
        assert logp == -np.inf and q.shape == (c["T"], c["W"]) and not q.any()


@pytest.mark.parametrize("W,n,K", [(2, 2, 3), (3, 3, 2), (2, 4, 5)])
def test_at_the_minimum_length_every_posterior_is_zero_or_one_per_boundary_rule(W, n, K):
    """T = K (n - 1) + 1 without skip arcs: every path advances one state per column, layer k holds columns k (n-1) ..
    (k+1)(n-1), and the shared boundary column belongs to the ENTERING layer.  So column t belongs to layer
    min(t // (n-1), K-1), whatever the words: q_t(k, .) sums to 1 there and to 0 elsewhere."""
    T = K * (n - 1) + 1
    c = layer_case(W, n, K, T, False, seed=1)
    q, logp, qk = restate(c)
    assert np.isfinite(logp)
    per_layer = qk.sum(axis=2)
    want = np.zeros((T, K))
    want[np.arange(T), np.minimum(np.arange(T) // (n - 1), K - 1)] = 1.0
    np.testing.assert_allclose(per_layer, want, rtol=0, atol=TOL)
    np.testing.assert_allclose(q.sum(axis=1), 1.0, rtol=0, atol=TOL)
    # one word: its posterior itself is 0 or 1
    c1 = layer_case(1, n, K, T, False, seed=1)
    _, _, qk1 = restate(c1)
    np.testing.assert_allclose(qk1[:, :, 0], want, rtol=0, atol=TOL)
    # ... and one frame less has no path
    assert restate(layer_case(W, n, K, T - 1, False, seed=1))[1] == -np.inf


def test_rows_sum_to_one_at_the_reference_shape_where_gamma_does_not():
    c = layer_case(11, 5, 7, 40, False, seed=2)
    post, logp, gsum = swept(c)
    assert np.isfinite(logp)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-11)     # (11 x 7 x 5 cells per row)
    assert post.min() >= 0.0 and post.max() <= 1.0 + TOL
    assert gsum.sum(axis=1).max() > 1.05, "the per-frame sum of gamma does not exceed 1: the correction is vacuous here"
    xpost, xlogp, _ = swept(c, np.longdouble)
    np.testing.assert_allclose(post, np.asarray(xpost, dtype=np.float64), rtol=0, atol=TOL)


def test_the_sweep_equals_the_formula():
    for shape in [(3, 3, 5, 17, True), (16, 2, 8, 12, False), (1, 4, 4, 15, True)]:
        c = layer_case(*shape, seed=3)
        q, logp, _ = restate(c)
        post, slogp, gsum = swept(c)
        assert abs(logp - slogp) <= TOL * abs(logp)
        np.testing.assert_allclose(post, q, rtol=0, atol=TOL)
        la, lb, gamma, _ = O.forward_backward(c["E"], c["nes"], c["trans"], c["ends"])
        per_word = np.stack([gamma[c["rw"] == w].sum(axis=0) for w in range(c["W"])], axis=1)
        np.testing.assert_allclose(gsum, per_word, rtol=0, atol=TOL)


@pytest.mark.parametrize("W,n,T,skip", [(3, 2, 6, False), (2, 3, 8, True), (3, 3, 9, False)])
def test_mixture_identity_against_the_loop_grammar(W, n, T, skip):
    """word_penalty = 0: q_loop_t(w) = sum_K exp(logP_K - logP_loop) q^K_t(w) and logP_loop = LSE_K logP_K, K = 1 .. 9
    (a path of the loop grammar has some number K of words and is a path of exactly the K-layer lattice)."""
    rng = np.random.default_rng(2900 + 100 * W + 10 * n + skip)
    wt = [word_trans(rng, n, skip) for _ in range(W)]
    costs = rng.uniform(0.5, 6.0, size=(T, W * n))
    lnes, lrw, lrl, ltrans, lends = O.loop_grammar(wt, n, 0.0)
    LE = np.where(lnes[:, None], 0.0, costs[:, np.where(lnes, 0, lrw * n + lrl)].T)
    lq, llogp = loop_word_posteriors(LE, lnes, lrw, ltrans, lends, W, n)
    qs, lps = [], []
    for K in range(1, 10):
        rw, rs, nes, trans, ends = layers_graph(wt, n, K)
        q, logp, _ = word_posteriors_layers(emissions(costs, rw, rs, n), nes, trans, ends, W, n, K)
        qs.append(q)
        lps.append(logp)
    assert sum(np.isfinite(lp) for lp in lps) >= 2
    tot = O._lse(lps)
    assert abs(tot - llogp) <= TOL * abs(llogp)
    mix = sum(np.exp(lp - tot) * q for q, lp in zip(qs, lps) if np.isfinite(lp))
    print("max |mixture - loop|: %.3g" % np.abs(mix - lq).max())
    np.testing.assert_allclose(mix, lq, rtol=0, atol=TOL)


@pytest.mark.parametrize("n,skip,T", [(2, False, 5), (3, True, 7)])
def test_one_layer_is_the_loop_form_restricted_to_one_word(n, skip, T):
    """K = 1: the utterance is exactly one word.  Its posterior is the mixture over the words' chains: q_t(w) = P(word w
    | x) in every column -- which is also what the one-word loop paths of each word give, weighted by their log P."""
    W = 3
    c = layer_case(W, n, 1, T, skip, seed=4)
    q, logp, _ = restate(c)
    # word w alone as a one-layer lattice: the forward score of its chain
    lps = []
    for w in range(W):
        rw, rs, nes, trans, ends = layers_graph([c["wt"][w]], n, 1)
        E = emissions(c["costs"][:, w * n:(w + 1) * n], rw, rs, n)
        q1, lp1, _ = word_posteriors_layers(E, nes, trans, ends, 1, n, 1)
        np.testing.assert_allclose(q1, 1.0, rtol=0, atol=TOL)
        # ... which is the one-word loop grammar's path set cut down to a single word: one layer has no loop to take
        lnes, lrw, lrl, ltrans, lends = O.loop_grammar([c["wt"][w]], n, np.inf)
        LE = np.where(lnes[:, None], 0.0, c["costs"][:, w * n + np.where(lnes, 0, lrl)].T)
        lq, llp = loop_word_posteriors(LE, lnes, lrw, ltrans, lends, 1, n)
        assert abs(llp - lp1) <= TOL * abs(lp1)
        np.testing.assert_allclose(lq, q1, rtol=0, atol=TOL)
        lps.append(lp1)
    assert abs(O._lse(lps) - logp) <= TOL * abs(logp)
    want = np.exp(np.array(lps) - logp)
    np.testing.assert_allclose(q, np.broadcast_to(want, q.shape), rtol=0, atol=TOL)


def test_the_extended_precision_recursion_is_the_oracles():
    c = layer_case(2, 3, 3, 9, True, seed=5)
    la, lb, gamma, logp = O.forward_backward(c["E"], c["nes"], c["trans"], c["ends"])
    xa, xb, xg, xlogp = forward_backward(c["E"], c["nes"], c["trans"], c["ends"], dtype=np.longdouble)
    assert xa.dtype == np.longdouble
    for x, y in ((xa, la), (xb, lb)):
        fin = np.isfinite(y)
        np.testing.assert_array_equal(np.isfinite(x), fin)
        np.testing.assert_allclose(np.asarray(x[fin], dtype=np.float64), y[fin], rtol=TOL, atol=TOL)
    q, qk = q_from_matrices(xa, xb, xlogp, c["trans"], c["W"], c["n"], c["K"])
    np.testing.assert_allclose(np.asarray(q, dtype=np.float64), restate(c)[0], rtol=0, atol=TOL)


def test_header_binding_and_library_have_the_entry(built_library):
    from sr.recognition import _hip
    raw = open(os.path.join(ROOT, "include", "gmmhmm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+gh_word_posteriors_layers\s*\(", text)
    doc = raw[raw.index("word posteriors and per-word confidence (K-layer lattice)"):raw.index("int gh_word_posteriors_layers")]
    assert "NOT in the reference" in doc and "NES_{k+1}" in doc
    assert "gh_word_posteriors_layers" in _hip.SIGNATURES
    assert _hip.SIGNATURES["gh_word_posteriors_layers"] == _hip.SIGNATURES["gh_word_posteriors"]
    res, args = _hip.SIGNATURES["gh_word_posteriors_layers"]
    assert res is ctypes.c_int and len(args) == 10
    assert hasattr(ctypes.CDLL(built_library), "gh_word_posteriors_layers")
    assert callable(getattr(_hip.Lattices, "word_posteriors_layers"))


# ----------------------------------------------------------------------------------------------------------------------
class LayersRecordingLattices(RecordingLattices):
    def word_posteriors_layers(self, batch, labels=None, begins=None, want_post=True):
        type(self).reached.append("word_posteriors_layers")
        return dict(logp=np.zeros(batch.U), post=np.zeros((batch.N, 1)), confidence=[np.zeros(len(l)) for l in (labels or [])])


XS_SEED = 21


def _xs(rng):
    return [rng.normal(size=(12, 3)), rng.normal(size=(9, 3))]


def test_without_the_keyword_a_layers_decoder_is_refused_as_before(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(XS_SEED)
    xs = _xs(rng)
    dec = ContinuousDecoder(make_models(rng, 3, 3), n_layers=2)
    b = _hip.Batch(dec.ctx, xs)
    made = CountingBatch.made
    for kw in ({}, dict(layers=False), dict(lm=True), dict(lm=True, layers=False)):
        for call in (lambda: dec.decode_batch(b, want_confidence=True, **kw), lambda: dec.word_posteriors(b, **kw),
                     lambda: dec.decode(xs, want_confidence=True, **kw)):
            with pytest.raises(_hip.Unsupported, match="K-layer lattice"):
                call()
    assert CountingBatch.made == made and CountingBatch.scored == 0 and UntouchedLattices.calls == 0


def test_with_the_keyword_the_scope_refusals_keep_distinct_sentences(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(XS_SEED + 1)
    xs = _xs(rng)
    beamed = ContinuousDecoder(make_models(rng, 3, 3), n_layers=2)
    beamed.lat.set_beam(4)
    cases = [(ContinuousDecoder(make_models(rng, 17, 2), n_layers=2), "up to 16 words per layer, not 17"),
             (ContinuousDecoder(make_models(rng, 2, 2), n_layers=9), "up to 8 layers, not 9"),
             (ContinuousDecoder(make_models(rng, 2, 12), n_layers=2), "2 to 8 states, not 12"),
             (ContinuousDecoder(make_models(rng, 2, 16), n_layers=2), "2 to 8 states, not 16"),
             (beamed, "rank beam")]
    sentences = set()
    for dec, hint in cases:
        b = _hip.Batch(dec.ctx, xs)
        made = CountingBatch.made
        for call in (lambda: dec.decode_batch(b, want_confidence=True, layers=True), lambda: dec.word_posteriors(b, layers=True),
                     lambda: dec.decode(xs, want_confidence=True, layers=True)):
            with pytest.raises(_hip.Unsupported, match=hint) as e:
                call()
            sentences.add(re.sub(r"not 1[26]$", "not N", str(e.value)))
        assert CountingBatch.made == made and CountingBatch.scored == 0 and UntouchedLattices.calls == 0
    assert len(sentences) == 4                                              # words, layers, states (12 and 16), beam
    dec = ContinuousDecoder(make_models(rng, 3, 3), n_layers=2)
    with pytest.raises(ValueError):
        dec.decode_batch(_hip.Batch(dec.ctx, xs), want_path=True, want_confidence=True, layers=True)
    assert UntouchedLattices.calls == 0
    # a bigram decoder still needs lm=True
    bigram = ContinuousDecoder(make_models(rng, 3, 3), grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3)))
    with pytest.raises(_hip.Unsupported, match="bigram grammar"):
        bigram.decode_batch(_hip.Batch(bigram.ctx, xs), want_confidence=True, layers=True)
    # the online decoders do not take the keyword
    from sr.recognition import batch as B
    for name in ("OnlineDecoder", "OnlineBigramDecoder", "OnlineLayersDecoder"):
        for meth, fn in inspect.getmembers(getattr(B, name), callable):
            if meth.startswith("__") and meth != "__init__":
                continue
            assert "layers" not in inspect.signature(fn).parameters, (name, meth)
    for meth in ("online", "online_bigram", "online_layers"):
        assert "layers" not in inspect.signature(getattr(ContinuousDecoder, meth)).parameters


def test_the_keyword_routes_by_grammar(fake_backend):
    """layers=True on a layers decoder reaches `word_posteriors_layers`; on a loop decoder `word_posteriors`, on a bigram
    decoder with lm=True `word_posteriors_bigram`, as without it; without want_confidence it changes nothing."""
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    fake_backend.setattr(_hip, "Lattices", LayersRecordingLattices)
    rng = np.random.default_rng(XS_SEED + 2)
    hmms = make_models(rng, 3, 3)
    xs = _xs(rng)
    layers = ContinuousDecoder(hmms, n_layers=2)
    loop = ContinuousDecoder(hmms, grammar="loop")
    bigram = ContinuousDecoder(hmms, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3)))
    for dec, kw, want in ((layers, dict(layers=True), "word_posteriors_layers"), (layers, dict(layers=True, lm=True), "word_posteriors_layers"),
                          (loop, dict(layers=True), "word_posteriors"), (bigram, dict(layers=True, lm=True), "word_posteriors_bigram")):
        del RecordingLattices.reached[:]
        b = _hip.Batch(dec.ctx, xs)
        words, r = dec.decode_batch(b, want_confidence=True, **kw)
        timed_words, timed = dec.decode_batch(b, want_times=True)
        assert words == timed_words and "confidence" in r and "logp" in r and "confidence" not in timed
        for u in range(len(xs)):
            np.testing.assert_array_equal(r["begins"][u], timed["begins"][u])
        dec.word_posteriors(b, **kw)
        w3, b3, c3 = dec.decode(xs, want_confidence=True, **kw)
        assert w3 == words and RecordingLattices.reached == [want] * 3
        del RecordingLattices.reached[:]
        plain_words, plain = dec.decode_batch(b, **kw)
        assert plain_words == dec.decode_batch(b)[0] == dec.decode(xs, **kw) and "confidence" not in plain
        assert dec.decode(xs, want_times=True, **kw)[0] == words
        assert RecordingLattices.reached == []


def test_the_posteriorgram_is_sized_from_the_graph():
    from sr.recognition import _hip
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice
    rng = np.random.default_rng(XS_SEED + 3)
    for W, n, K in ((11, 5, 7), (1, 2, 1), (16, 8, 8), (3, 3, 4)):
        graph, _ = packed_lattice([word_trans(rng, n, False) for _ in range(W)], n, [list(range(W))] * K)
        lat = _hip.Lattices.__new__(_hip.Lattices)
        lat._row_state0 = np.asarray(graph["row_state"], dtype=np.int64)
        lat._row0_fanout = int(np.count_nonzero(np.asarray(graph["arc_from"]) == 0))
        assert lat._layers_words() == W and lat._loop_words() is None
        lat.h = None
    graph, _ = packed_loop_lattice([word_trans(rng, 3, False) for _ in range(4)], 3, 0.0)
    lat = _hip.Lattices.__new__(_hip.Lattices)
    lat._row_state0 = np.asarray(graph["row_state"], dtype=np.int64)
    lat._row0_fanout = int(np.count_nonzero(np.asarray(graph["arc_from"]) == 0))
    assert lat._layers_words() is None and lat._loop_words() == 4
    lat.h = None
