# -*- coding: utf-8 -*-
"""Word posteriors and per-word confidence of the loop grammar, on the host (no GPU).

1. The restatement (tests/word_posteriors_ref.py: q from `O.forward_backward`) against brute-force path enumeration at
   2 words x 2 states (T = 2 .. 6) and at 3 x 3 with skip arcs (T <= 7); its rows sum to one at 17 x 5, T = 40.
2. No path (T = 1, T < n): log P = -inf, zero rows, confidences that are safe on an empty decode.
3. The same word twice in a row: confidences stay <= 1 while the per-word sum of gamma (what `occ` gives) exceeds 1 on
   the boundary frame.
4. gh_word_posteriors is in the header, in the ctypes table and exported.
5. `ContinuousDecoder` refuses the bigram grammar, the K-layer lattice, a beam and 12-state words before the backend is
   touched (a test double of `Lattices` defined here), each with a sentence of its own."""
import ctypes
import os
import re

import numpy as np
import pytest

import fake_hip
from conftest import ROOT
from oracle import ref_numpy as O
from word_posteriors_ref import brute_force, confidence, word_posteriors


def word_trans(rng, n, skip):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.1, 2.0)
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.1, 2.0)
        if skip and i < n - 2:
            t[i + 2, i] = rng.uniform(0.1, 2.0)
    return t


def loop_case(W, n, skip, T, penalty=0.0, seed=0):
    rng = np.random.default_rng(700 + 100 * W + 10 * n + skip + seed)
    nes, rw, rs, dense, ends = O.loop_grammar([word_trans(rng, n, skip) for _ in range(W)], n, penalty)
    E = np.where(nes[:, None], 0.0, rng.uniform(0.2, 4.0, size=(len(nes), T)))
    return nes, rw, dense, ends, E


@pytest.mark.parametrize("W,n,skip,Ts", [(2, 2, False, (2, 3, 4, 5, 6)), (3, 3, True, (2, 3, 5, 7))])
def test_restatement_equals_brute_force(W, n, skip, Ts):
    for T in Ts:
        nes, rw, dense, ends, E = loop_case(W, n, skip, T, penalty=0.3)
        post, logp = word_posteriors(E, nes, rw, dense, ends, W, n)
        bf, bf_logp = brute_force(E, nes, rw, dense, ends, W)
        assert np.isfinite(logp)
        np.testing.assert_allclose(logp, bf_logp, rtol=1e-12)
        np.testing.assert_allclose(post, bf, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert post.min() >= 0.0 and post.max() <= 1.0 + 1e-12


def test_rows_sum_to_one_where_the_sum_of_gamma_does_not():
    W, n, T = 17, 5, 40
    nes, rw, dense, ends, E = loop_case(W, n, False, T)
    post, logp = word_posteriors(E, nes, rw, dense, ends, W, n)
    assert np.isfinite(logp)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    gamma = O.forward_backward(E, nes, dense, ends)[2]
    assert gamma[~nes].sum(axis=0).max() > 1.05                           # a boundary frame is occupied twice


@pytest.mark.parametrize("W,n,T", [(2, 2, 1), (3, 4, 1), (3, 4, 3), (2, 5, 4)])
def test_no_path(W, n, T):
    nes, rw, dense, ends, E = loop_case(W, n, False, T)
    post, logp = word_posteriors(E, nes, rw, dense, ends, W, n)
    assert logp == -np.inf and post.shape == (T, W) and not post.any()
    assert brute_force(E, nes, rw, dense, ends, W)[1] == -np.inf
    assert confidence(post, [], [], T).shape == (0,)
    np.testing.assert_array_equal(confidence(post, [1], [0], T), [0.0])


def test_a_repeated_word_keeps_its_confidences_below_one():
    """One word, decoded twice in a row: the boundary frame is occupied by both passes (per-word gamma sum 2 there when
    the decode is certain), the word posterior of the only word is 1 in every frame."""
    from sr.recognition.batch import path_to_word_times
    W, n, T = 1, 3, 9
    rng = np.random.default_rng(5)
    nes, rw, rs, dense, ends = O.loop_grammar([word_trans(rng, n, False)], n, 0.0)
    # emissions that pull the path through the word twice: states 0 1 2 | 0 1 2, the boundary frame scored by 2 then 0
    E = np.full((len(nes), T), 6.0)
    E[nes] = 0.0
    row = {0: 1 + W * (n - 1) + 1, 1: 1, 2: 2}
    for t, s in enumerate([0, 0, 1, 2, 2, 0, 1, 1, 2]):
        E[row[s], t] = 0.1
    E[row[0], 4] = 0.1                                                    # frame 4: last state of pass one, first of pass two
    costs, path = O.decode_states(E, nes, dense, end_points=[[int(e), -1] for e in ends])
    row_state = np.where(nes, -1, rw * n + rs)
    words, begins = path_to_word_times(path, row_state, n)
    assert words == [0, 0] and begins[0] == 0 and 0 < begins[1] < T
    post, logp = word_posteriors(E, nes, rw, dense, ends, W, n)
    gamma = O.forward_backward(E, nes, dense, ends)[2]
    per_word = gamma[~nes].sum(axis=0)
    assert per_word[begins[1]] > 1.5                                      # what `occ` summed per word would report
    conf = confidence(post, words, begins, T)
    assert conf.shape == (2,) and np.all(conf <= 1.0 + 1e-12) and np.all(conf > 0.99)
    np.testing.assert_allclose(post[:, 0], 1.0, rtol=0, atol=1e-12)


def test_header_binding_and_library_have_the_entry(built_library):
    from sr.recognition import _hip
    raw = open(os.path.join(ROOT, "include", "gmmhmm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+gh_word_posteriors\s*\(", text)
    assert "NOT in the reference" in raw[raw.index("word posteriors and per-word confidence"):raw.index("int gh_word_posteriors")]
    assert "gh_word_posteriors" in _hip.SIGNATURES
    res, args = _hip.SIGNATURES["gh_word_posteriors"]
    assert res is ctypes.c_int and len(args) == 10
    assert hasattr(ctypes.CDLL(built_library), "gh_word_posteriors")
    assert callable(getattr(_hip.Lattices, "word_posteriors"))


# ----------------------------------------------------------------------------------------------------------------------
class UntouchedLattices(fake_hip.Lattices):
    """Test double of `_hip.Lattices`: counts what reaches the backend; the posteriors must never be asked of it."""
    calls = 0

    def viterbi_labels(self, *a, **k):
        type(self).calls += 1
        raise AssertionError("the decoder must refuse before the backend is asked")

    word_posteriors = forward_backward = viterbi = viterbi_labels


class CountingBatch(fake_hip.Batch):
    made = 0
    scored = 0

    def __init__(self, *a, **k):
        type(self).made += 1
        super().__init__(*a, **k)

    def loglik(self, *a, **k):
        type(self).scored += 1
        return super().loglik(*a, **k)


@pytest.fixture
def fake_backend(monkeypatch, built_library):
    from sr.recognition import _hip, _pack
    fake_hip.install(monkeypatch, _hip)
    monkeypatch.setattr(_hip, "Lattices", UntouchedLattices)
    monkeypatch.setattr(_hip, "Batch", CountingBatch)
    monkeypatch.setattr(UntouchedLattices, "calls", 0)
    monkeypatch.setattr(CountingBatch, "made", 0)
    monkeypatch.setattr(CountingBatch, "scored", 0)
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()
    yield
    _pack._gmm_cache.clear()
    _pack._lat_cache.clear()


def make_models(rng, W, n, M=2, D=3):
    import sr.recognition as R
    hmms = []
    for i in range(W):
        h = R.HMM(n)
        h.gmm_states = []
        for s in range(n):
            g = R.GMM(rng.normal(size=D), rng.uniform(0.5, 1.5, size=D), M)
            g.update_models(rng.normal(size=(M, D)), rng.uniform(0.5, 1.5, size=(M, D)), rng.dirichlet(np.ones(M)))
            h.gmm_states.append(g)
        h.transitions = word_trans(rng, n, False)
        hmms.append(h)
    return hmms


def test_refusals_fire_before_the_backend_is_touched(fake_backend):
    from sr.recognition import _hip
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(11)
    hmms = make_models(rng, 3, 3)
    xs = [rng.normal(size=(12, 3)), rng.normal(size=(9, 3))]
    beamed = ContinuousDecoder(hmms, grammar="loop")
    beamed.lat.set_beam(4)
    cases = [(ContinuousDecoder(hmms, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3))), "bigram grammar"),
             (ContinuousDecoder(hmms, n_layers=2), "K-layer lattice"),
             (beamed, "rank beam"),
             (ContinuousDecoder(make_models(rng, 2, 12), grammar="loop"), "2 to 8 states, not 12")]
    sentences = set()
    for dec, hint in cases:
        b = _hip.Batch(dec.ctx, xs)
        made = CountingBatch.made
        for call in (lambda: dec.decode_batch(b, want_confidence=True), lambda: dec.word_posteriors(b),
                     lambda: dec.decode(xs, want_confidence=True)):
            with pytest.raises(_hip.Unsupported, match=hint) as e:
                call()
            sentences.add(str(e.value))
        assert CountingBatch.made == made and CountingBatch.scored == 0 and UntouchedLattices.calls == 0
    assert len(sentences) == len(cases)                                   # a sentence of its own per case
    # the keyword belongs to the label decode
    dec = ContinuousDecoder(hmms, grammar="loop")
    with pytest.raises(ValueError):
        dec.decode_batch(_hip.Batch(dec.ctx, xs), want_path=True, want_confidence=True)
    assert UntouchedLattices.calls == 0
    # the online decoders do not take it
    import inspect
    from sr.recognition import batch as B
    for name in ("OnlineDecoder", "OnlineBigramDecoder", "OnlineLayersDecoder"):
        for meth in ("result", "commit", "tail", "finish"):
            fn = getattr(getattr(B, name), meth, None)
            if fn is not None:
                assert "want_confidence" not in inspect.signature(fn).parameters
