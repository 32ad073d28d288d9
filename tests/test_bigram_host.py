# -*- coding: utf-8 -*-
"""The bigram grammar on the host: the reference's own decode of the graph (G20) against the oracle, the two graph
builders against each other and against G20's arcs, the uniform-cost case against the loop grammar, `BigramModel`'s
counts / costs / errors, and a decode in which a forbidden pair changes the answer."""
import warnings

import numpy as np
import pytest

from conftest import load_golden
from oracle import ref_numpy as O

RT = 1e-12      # tests/test_oracle_golden.py: fp64 values against the reference


@pytest.fixture(scope="module")
def g20():
    return load_golden("G20_bigram_grammar")


def _dense(R, to, frm, cost):
    t = np.full((R, R), np.inf)
    t[to, frm] = cost
    return t


def _decode(E, nes, trans, ends):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O.decode_states(E, nes, trans, end_points=[[e, -1] for e in ends])


class _Word:
    """What the object-level builders read of an HMM: the state objects and the transition costs."""

    def __init__(self, states, transitions):
        self.gmm_states = states
        self.transitions = transitions


def word_trans(rng, n, skip=False):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.05, 0.6) if i < n - 1 else 0.0
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.8, 2.5)
        if skip and i < n - 2:
            t[i + 2, i] = rng.uniform(1.5, 4.0)
    return t


@pytest.mark.parametrize("case", [0, 1, 2])
def test_G20_bigram_grammar(g20, case):
    """The reference's decode_hmm_states on the bigram graph: the oracle reproduces its cost matrices, paths and digits
    from the arrays as stored (c2: tied predecessor words, the first minimum decides)."""
    g, pp = g20, "c%d_" % case
    means, vars_, w = g[pp + "means"], g[pp + "vars"], g[pp + "w"]
    rw, rs, ends = g[pp + "row_word"], g[pp + "row_state"], g[pp + "ends"]
    R = len(rw)
    nes = rw < 0
    trans = _dense(R, g[pp + "arc_to"], g[pp + "arc_from"], g[pp + "arc_cost"])
    states = [None if nes[r] else (means[rw[r], rs[r]], vars_[rw[r], rs[r]], w[rw[r], rs[r]]) for r in range(R)]
    for u in range(int(g["n_utts"])):
        costs, path = _decode(O.emission_matrix(g[pp + "x%d" % u], states), nes, trans, ends)
        np.testing.assert_allclose(costs, g[pp + "costs%d" % u], rtol=RT, atol=0.0)
        np.testing.assert_array_equal(path, g[pp + "path%d" % u])
        assert O.path_to_words(path, nes, rw) == list(g[pp + "digits%d" % u])


def test_G20_tie_case_has_ties(g20):
    """c2 is only worth its place if two predecessor words really tie at an entry row of the decoded path."""
    g, pp = g20, "c2_"
    rw, rs = g[pp + "row_word"], g[pp + "row_state"]
    R, W = len(rw), int(rw.max()) + 1
    n = int(rs.max()) + 1
    trans = _dense(R, g[pp + "arc_to"], g[pp + "arc_from"], g[pp + "arc_cost"])
    first = 1 + W * (n - 1)
    ties = 0
    for u in range(int(g["n_utts"])):
        costs = g[pp + "costs%d" % u]
        for r, c in g[pp + "path%d" % u]:
            if first <= r < first + W:
                cand = trans[r] + costs[:, c]
                ties += int(np.sum(cand == cand.min()) > 1)
    assert ties > 0


@pytest.mark.parametrize("case", [0, 1, 2])
def test_builders_agree_with_G20(g20, case):
    """build_bigram_grammar's dense matrix, packed_bigram_lattice's arc list and the arcs the reference decoded (G20)
    are the same graph: same rows, same non-emitting rows, same ends, bit-equal costs."""
    from sr.recognition.continuous_speech import build_bigram_grammar, packed_bigram_lattice
    from sr.recognition.hmm_state import NES
    g, pp = g20, "c%d_" % case
    rw, rs = g[pp + "row_word"], g[pp + "row_state"]
    W, n = int(rw.max()) + 1, int(rs.max()) + 1
    wt = g["word_trans"]
    words = [_Word([("state", i, s) for s in range(n)], wt) for i in range(W)]
    seq, trans, ends = build_bigram_grammar(words, g[pp + "B"], g[pp + "init"])
    R = len(rw)
    np.testing.assert_array_equal(trans, _dense(R, g[pp + "arc_to"], g[pp + "arc_from"], g[pp + "arc_cost"]))
    np.testing.assert_array_equal(ends, g[pp + "ends"])
    for r in range(R):
        if rw[r] < 0:
            assert isinstance(seq[r], NES)
        else:
            assert seq[r] == ("state", int(rw[r]), int(rs[r]))
    graph, nes_rows = packed_bigram_lattice([wt] * W, n, g[pp + "B"], g[pp + "init"])
    np.testing.assert_array_equal(_dense(R, graph["arc_to"], graph["arc_from"], graph["arc_cost"]), trans)
    assert len(graph["arc_to"]) == int(np.sum(~np.isinf(trans)))            # every arc once
    np.testing.assert_array_equal(graph["row_state"], np.where(rw < 0, -1, rw * n + rs))
    np.testing.assert_array_equal(graph["end_rows"], g[pp + "ends"])
    np.testing.assert_array_equal(graph["start_rows"], [0])
    np.testing.assert_array_equal(nes_rows, np.flatnonzero(rw < 0))
    g2, _ = packed_bigram_lattice([wt] * W, n, g[pp + "B"], g[pp + "init"], state_base=[100, 7, 50, 20])
    np.testing.assert_array_equal(g2["row_state"], np.where(rw < 0, -1, np.array([100, 7, 50, 20])[rw] + rs))


def test_builder_errors():
    from sr.recognition.continuous_speech import build_bigram_grammar, packed_bigram_lattice
    rng = np.random.default_rng(1)
    wt = [word_trans(rng, 3) for _ in range(3)]
    B = np.ones((3, 3))
    for bad in (np.ones((3, 2)), np.ones((4, 4)), np.ones(3)):
        with pytest.raises(ValueError):
            packed_bigram_lattice(wt, 3, bad)
    for v in (np.nan, -np.inf):
        Bb = B.copy()
        Bb[1, 2] = v
        with pytest.raises(ValueError):
            packed_bigram_lattice(wt, 3, Bb)
        with pytest.raises(ValueError):
            packed_bigram_lattice(wt, 3, B, initial=[0.0, v, 0.0])
        with pytest.raises(ValueError):
            build_bigram_grammar([_Word([0, 1, 2], t) for t in wt], Bb)
    with pytest.raises(ValueError):
        packed_bigram_lattice(wt, 3, B, initial=[0.0, 1.0])
    with pytest.raises(ValueError):
        packed_bigram_lattice([np.zeros((1, 1))] * 3, 1, B)
    with pytest.raises(ValueError):
        build_bigram_grammar([_Word([0], np.zeros((1, 1)))] * 3, B)
    # +inf is a legal cost: the arc is left out
    Bi = B.copy()
    Bi[0, 1] = np.inf
    graph, _ = packed_bigram_lattice(wt, 3, Bi, initial=[0.0, np.inf, 0.0])
    assert np.all(np.isfinite(graph["arc_cost"]))


@pytest.mark.parametrize("W,n,skip,p", [(4, 3, False, 0.0), (3, 5, True, 2.5), (6, 2, False, 1.25)])
def test_constant_bigram_is_the_loop_grammar(W, n, skip, p):
    """B = p everywhere, init = 0: end costs BIT-EQUAL to the loop grammar with word_penalty = p, same word strings."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(100 * W + n)
    wt = [word_trans(rng, n, skip) for _ in range(W)]
    graph, _ = packed_bigram_lattice(wt, n, np.full((W, W), p))
    R = len(graph["row_state"])
    trans = _dense(R, graph["arc_to"], graph["arc_from"], graph["arc_cost"])
    nes = graph["row_state"] < 0
    rw = np.where(nes, -1, graph["row_state"] // n)
    lnes, lrw, lrs, ltrans, lends = O.loop_grammar(wt, n, p)
    lstate = np.where(lnes, -1, lrw * n + lrs)
    for u in range(12):
        T = int(rng.integers(2, 9 * n))
        nll = rng.uniform(0.5, 9.0, size=(T, W * n))
        E = np.where(nes[:, None], 0.0, nll[:, np.maximum(graph["row_state"], 0)].T)
        El = np.where(lnes[:, None], 0.0, nll[:, np.maximum(lstate, 0)].T)
        cb, pb = _decode(E, nes, trans, graph["end_rows"])
        cl, pl = _decode(El, lnes, ltrans, lends)
        np.testing.assert_array_equal(cb[graph["end_rows"], -1], cl[lends, -1])
        assert O.path_to_words(pb, nes, rw) == O.path_to_words(pl, lnes, lrw)


# ------------------------------------------------------------------------------------------------ BigramModel
def test_bigram_model_counts_and_costs():
    from sr.langmodel import BigramModel
    corpus = [[0, 1, 1], [1, 2], [0, 1], [], [2]]
    m = BigramModel(3, smoothing=0.5).fit(corpus)
    np.testing.assert_array_equal(m.start_counts, [2, 1, 1])
    np.testing.assert_array_equal(m.pair_counts, [[0, 2, 0], [0, 1, 1], [0, 0, 0]])
    init, B = m.costs()
    assert init.dtype == np.float64 and B.dtype == np.float64
    np.testing.assert_allclose(init, -np.log(np.array([2.5, 1.5, 1.5]) / 5.5), rtol=1e-15)
    np.testing.assert_allclose(B, -np.log(np.array([[0.5, 2.5, 0.5], [0.5, 1.5, 1.5], [0.5, 0.5, 0.5]]) /
                                          np.array([[3.5], [3.5], [1.5]])), rtol=1e-15)
    np.testing.assert_allclose(np.exp(-B).sum(axis=1), 1.0, rtol=1e-14)
    np.testing.assert_allclose(np.exp(-init).sum(), 1.0, rtol=1e-14)
    i2, B2 = m.costs(scale=3.0)
    np.testing.assert_array_equal(i2, 3.0 * init)
    np.testing.assert_array_equal(B2, 3.0 * B)
    # score = the sum of the arc costs along the word string
    assert m.score([]) == 0.0
    assert m.score([2]) == init[2]
    np.testing.assert_allclose(m.score([0, 1, 1, 2]), init[0] + B[0, 1] + B[1, 1] + B[1, 2], rtol=1e-15)
    np.testing.assert_allclose(m.score([0, 1], scale=2.0), 2.0 * (init[0] + B[0, 1]), rtol=1e-15)


def test_bigram_model_score_is_what_the_grammar_adds():
    """Decoding under the bigram grammar costs exactly `score(words)` more than the same path costs without a
    language model (B = 0, init = 0): the grammar adds the model's costs arc by arc."""
    from sr.langmodel import BigramModel
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(5)
    W, n = 3, 3
    m = BigramModel(W, smoothing=1.0).fit([[0, 1, 2, 1], [2, 2, 0], [1, 0]])
    init, B = m.costs()
    wt = [word_trans(rng, n) for _ in range(W)]
    graph, _ = packed_bigram_lattice(wt, n, B, init)
    free, _ = packed_bigram_lattice(wt, n, np.zeros((W, W)))
    R = len(graph["row_state"])
    nes = graph["row_state"] < 0
    rw = np.where(nes, -1, graph["row_state"] // n)
    for u in range(6):
        nll = rng.uniform(0.5, 9.0, size=(int(rng.integers(8, 30)), W * n))
        E = np.where(nes[:, None], 0.0, nll[:, np.maximum(graph["row_state"], 0)].T)
        costs, path = _decode(E, nes, _dense(R, graph["arc_to"], graph["arc_from"], graph["arc_cost"]), graph["end_rows"])
        words = O.path_to_words(path, nes, rw)
        # the same path, re-scored on the graph without language-model costs
        tf = _dense(R, free["arc_to"], free["arc_from"], free["arc_cost"])
        cells = [tuple(c) for c in path[::-1]]
        end = (int(graph["end_rows"][np.flatnonzero(costs[graph["end_rows"], -1] == costs[graph["end_rows"], -1].min())[-1]]), E.shape[1] - 1)
        cells.append(end)
        acoustic = E[cells[0]]
        for a, b in zip(cells[:-1], cells[1:]):
            acoustic += tf[b[0], a[0]] + E[b]
        np.testing.assert_allclose(costs[end], acoustic + m.score(words), rtol=1e-12)


def test_bigram_model_unseen_pairs_and_errors(tmp_path):
    from sr.langmodel import BigramModel
    import sr.langmodel as LM
    assert "BigramModel" in LM.__all__ if hasattr(LM, "__all__") else hasattr(LM, "BigramModel")
    m = BigramModel(3, smoothing=0).fit([[0, 1], [0, 1, 2]])
    init, B = m.costs()
    np.testing.assert_array_equal(np.isinf(init), [False, True, True])
    np.testing.assert_array_equal(np.isinf(B), [[True, False, True], [True, True, False], [True, True, True]])
    assert init[0] == 0.0 and B[0, 1] == 0.0 and B[1, 2] == 0.0
    assert m.score([0, 1, 2]) == 0.0 and np.isinf(m.score([1, 0]))
    with pytest.raises(ValueError):
        BigramModel(3, smoothing=-0.1)
    with pytest.raises(ValueError):
        BigramModel(3, smoothing=np.nan)
    with pytest.raises(ValueError):
        BigramModel(0)
    for bad in ([[0, 3]], [[-1]], [[0.5, 1.0]], [[[0, 1]]]):
        with pytest.raises(ValueError):
            BigramModel(3).fit(bad)
    for empty in ([], [[]], [[], []]):
        with pytest.raises(ValueError):
            BigramModel(3).fit(empty)
    with pytest.raises(ValueError):
        BigramModel(3).costs()
    with pytest.raises(ValueError):
        m.score([0, 7])
    with pytest.raises(ValueError):
        m.costs(scale=0.0)
    path = str(tmp_path / "bigram.npz")
    m2 = BigramModel(3, smoothing=0.25).fit([[2, 1, 0], [1, 1]])
    m2.save(path)
    m3 = BigramModel.load(path)
    assert m3.n_words == 3 and m3.smoothing == 0.25
    np.testing.assert_array_equal(m3.start_counts, m2.start_counts)
    np.testing.assert_array_equal(m3.pair_counts, m2.pair_counts)
    np.testing.assert_array_equal(m3.costs()[1], m2.costs()[1])


def test_forbidden_pair_is_never_decoded():
    """Utterances synthesised from the word pair (0, 1): the uniform loop grammar returns that pair; with B[0, 1] = +inf
    the decode never does -- the language model decides."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(21)
    W, n, D = 3, 3, 4
    means = rng.normal(size=(W, n, D)) * 3.0
    wt = [word_trans(rng, n) for _ in range(W)]
    B = np.full((W, W), 1.0)
    Bf = B.copy()
    Bf[0, 1] = np.inf
    got_pair = 0
    for u in range(10):
        segs = []
        for wd in (0, 1):
            Tw = int(rng.integers(2 * n, 4 * n))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            segs.append(means[wd, st] + 0.3 * rng.normal(size=(Tw, D)))
        x = np.concatenate(segs)
        nll = 0.5 * ((x[:, None, :] - means.reshape(W * n, D)[None]) ** 2).sum(axis=2)
        words = {}
        for name, cost in (("uniform", B), ("forbidden", Bf)):
            graph, _ = packed_bigram_lattice(wt, n, cost)
            R = len(graph["row_state"])
            nes = graph["row_state"] < 0
            rw = np.where(nes, -1, graph["row_state"] // n)
            E = np.where(nes[:, None], 0.0, nll[:, np.maximum(graph["row_state"], 0)].T)
            costs, path = _decode(E, nes, _dense(R, graph["arc_to"], graph["arc_from"], graph["arc_cost"]), graph["end_rows"])
            assert np.isfinite(costs[graph["end_rows"], -1]).any()
            words[name] = O.path_to_words(path, nes, rw)
        # the uniform case is the loop grammar with word_penalty 1
        lnes, lrw, lrs, ltrans, lends = O.loop_grammar(wt, n, 1.0)
        El = np.where(lnes[:, None], 0.0, nll[:, np.maximum(np.where(lnes, -1, lrw * n + lrs), 0)].T)
        assert O.path_to_words(_decode(El, lnes, ltrans, lends)[1], lnes, lrw) == words["uniform"]
        assert words["uniform"] == [0, 1]
        got_pair += 1
        f = words["forbidden"]
        assert all((a, b) != (0, 1) for a, b in zip(f[:-1], f[1:])), f
    assert got_pair == 10
