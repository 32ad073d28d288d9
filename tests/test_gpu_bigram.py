# -*- coding: utf-8 -*-
"""The bigram-form kernel (gh_viterbi_bigram.hip: four utterances per wave, lane = word, one entry row per word as a
16 x 16 min-plus step over DPP row broadcasts, 4-bit predecessor words in the decision records) against the reference's
goldens (G20), the oracle and the generic kernel, which implements the same decode_hmm_states semantics
(decode.py:80-146) by an entirely different route.

`Lattices.viterbi(batch)` with ONE graph for the whole batch takes the bigram-form kernel when the graph carries the
"bigram" form bit; GMMHMM_VITERBI=generic keeps it out."""
import contextlib
import os
import warnings

import numpy as np
import pytest

from conftest import load_golden
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@contextlib.contextmanager
def forced(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def word_trans(rng, n, skip=False, last_self=0.0, integer=False):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = (float(rng.integers(0, 2)) if integer else rng.uniform(0.05, 0.6)) if i < n - 1 else last_self
        if i < n - 1:
            t[i + 1, i] = float(rng.integers(1, 3)) if integer else rng.uniform(0.8, 2.5)
        if skip and i < n - 2 and rng.random() < 0.6:
            t[i + 2, i] = float(rng.integers(2, 4)) if integer else rng.uniform(1.5, 4.0)
    return t


def random_costs(rng, W, forbid):
    """B [W, W] with a fraction `forbid` of +inf entries -- but every word keeps at least one way in (a column without
    any arc is an entry row without origin, which the reference's back-trace cannot leave) -- and start costs with some
    +inf, at least one word finite."""
    B = rng.uniform(0.0, 4.0, size=(W, W))
    B[rng.random((W, W)) < forbid] = np.inf
    keep = rng.integers(0, W, size=W)
    B[keep, np.arange(W)] = rng.uniform(0.0, 4.0, size=W)
    init = rng.uniform(0.0, 2.0, size=W)
    init[rng.random(W) < 0.3] = np.inf
    init[int(rng.integers(0, W))] = rng.uniform(0.0, 2.0)
    return B, init


def make_model(rng, W, n, M=2, D=6):
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    return means, vars_, w


def make_utts(rng, means, vars_, U, short_every=9, max_words=6):
    W, n, M, D = means.shape
    xs = []
    for u in range(U):
        if short_every and u % short_every == 0:
            xs.append(rng.normal(size=(int(rng.integers(2, max(3, n))), D)) * 2.0)      # shorter than any word
            continue
        segs = []
        for wd in rng.integers(0, W, size=rng.integers(1, max_words + 1)):
            Tw = int(rng.integers(n, 3 * n + 4))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            comp = rng.integers(0, M, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D)))
        xs.append(np.concatenate(segs))
    return xs


def dense_of(graph):
    R = len(graph["row_state"])
    t = np.full((R, R), np.inf)
    t[graph["arc_to"], graph["arc_from"]] = graph["arc_cost"]
    return t


def oracle_decode(graph, nll_u, beam=None):
    nes = graph["row_state"] < 0
    E = np.zeros((len(nes), len(nll_u)))
    E[~nes] = nll_u[:, graph["row_state"][~nes]].T
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O.decode_states(E, nes, dense_of(graph), end_points=[[int(e), -1] for e in graph["end_rows"]], beam=beam)


def oracle_best_end(costs, ends):
    ec = costs[np.asarray(ends), -1]
    return int(np.flatnonzero(ec == ec.min())[-1])           # the last of equal minima (decode.py:129-134)


def check_against_oracle(graph, r, nll, offsets, rtol, paths=True):
    ends = np.asarray(graph["end_rows"])
    for u in range(len(offsets) - 1):
        costs, path = oracle_decode(graph, nll[offsets[u]:offsets[u + 1]])
        ec = costs[ends, -1]
        fin = np.isfinite(ec)
        np.testing.assert_array_equal(np.isfinite(r["end_cost"][u]), fin)
        np.testing.assert_allclose(r["end_cost"][u][fin], ec[fin], rtol=rtol)
        if paths:
            assert int(r["best_end"][u]) == oracle_best_end(costs, ends)
            np.testing.assert_array_equal(r["paths"][u], path)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bigram_kernel_reference_goldens(hip, ctx, dtype):
    """G20: the bigram graph decoded by the reference's own decode_hmm_states -- end costs, BIT-EXACT paths and digits
    through the bigram-form kernel, for random, forbidden and tied (c2) costs."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    g = load_golden("G20_bigram_grammar")
    wt = g["word_trans"]
    U = int(g["n_utts"])
    for case in range(int(g["n_cases"])):
        pp = "c%d_" % case
        means, vars_, w = g[pp + "means"], g[pp + "vars"], g[pp + "w"]
        W, n, M, D = means.shape
        gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
        graph = packed_bigram_lattice([wt] * W, n, g[pp + "B"], g[pp + "init"])[0]
        lat = hip.Lattices(ctx, [graph])
        assert "bigram" in lat.forms()
        b = hip.Batch(ctx, [g[pp + "x%d" % u] for u in range(U)], dtype=dtype)
        b.loglik(gmm, fetch=False)
        r = lat.viterbi(b, want_path=True)
        rw = g[pp + "row_word"]
        ends = np.asarray(graph["end_rows"])
        for u in range(U):
            ref = g[pp + "costs%d" % u][ends, -1]
            fin = np.isfinite(ref)
            np.testing.assert_array_equal(np.isfinite(r["end_cost"][u]), fin)
            np.testing.assert_allclose(r["end_cost"][u][fin], ref[fin], rtol=1e-10 if dtype == np.float64 else 1e-5)
            np.testing.assert_array_equal(r["paths"][u], g[pp + "path%d" % u])
            assert O.path_to_words(r["paths"][u], rw < 0, rw) == list(g[pp + "digits%d" % u])
        b.close(); lat.close(); gmm.close()


# every W x n x skip of the plan (words of two states have no s-2 arc: the "skip" case is then a second draw of the
# plain one), plus the wide word models the kernel is instantiated for and a few sizes in between
SWEEP = [(W, n, skip) for W in (2, 5, 11, 16) for n in (2, 3, 5, 8) for skip in (False, True)]
SWEEP += [(4, 12, False), (3, 12, True), (16, 12, True), (5, 16, False), (16, 16, False), (7, 4, True), (9, 6, False), (13, 7, True)]


@pytest.mark.parametrize("W,n,skip", SWEEP)
def test_bigram_kernel_equals_generic_kernel_and_oracle(hip, ctx, W, n, skip):
    """Random word models and bigram costs (10-30 % forbidden pairs, some words that cannot start): ragged utterances of
    1 .. 6 words, a few too short for even one word, a count that is not a multiple of the four utterances of a wave.
    Bigram-form kernel == generic kernel == oracle: end costs to 1e-10, best ends and paths identical, labels follow."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    from sr.recognition.batch import path_to_words
    rng = np.random.default_rng(1000 * W + 10 * n + skip)
    means, vars_, w = make_model(rng, W, n)
    wt = [word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)]
    B, init = random_costs(rng, W, rng.uniform(0.1, 0.3))
    xs = make_utts(rng, means, vars_, 41)
    M, D = means.shape[2:]
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    lat = hip.Lattices(ctx, [graph])
    assert "bigram" in lat.forms()
    row_word = np.where(graph["row_state"] >= 0, graph["row_state"] // n, -1).astype(np.int32)
    for dtype in (np.float64, np.float32):
        b = hip.Batch(ctx, xs, dtype=dtype)
        nll = np.asarray(b.loglik(gmm), dtype=np.float64)
        fast = lat.viterbi(b, want_path=True)
        with forced(GMMHMM_VITERBI="generic"):
            gen = lat.viterbi(b, want_path=True)
            lgen = lat.viterbi_labels(b, row_word)
        np.testing.assert_array_equal(np.isinf(fast["end_cost_flat"]), np.isinf(gen["end_cost_flat"]))
        fin = np.isfinite(gen["end_cost_flat"])
        np.testing.assert_allclose(fast["end_cost_flat"][fin], gen["end_cost_flat"][fin], rtol=1e-10)
        np.testing.assert_array_equal(fast["best_end"], gen["best_end"])
        for u in range(b.U):
            np.testing.assert_array_equal(fast["paths"][u], gen["paths"][u])
        check_against_oracle(graph, fast, nll, b.offsets, rtol=1e-10)
        unreachable = [u for u in range(b.U) if not np.isfinite(fast["end_cost"][u]).any()]
        if not skip and n > 2:
            assert unreachable, "the sweep is meant to hold utterances that no word fits"
        nopath = lat.viterbi(b, want_path=False)
        np.testing.assert_array_equal(nopath["end_cost_flat"], fast["end_cost_flat"])
        np.testing.assert_array_equal(nopath["best_end"], fast["best_end"])
        la = lat.viterbi_labels(b, row_word)
        lc = lat.viterbi_labels(b, row_word, as_lists=False)
        for u in range(b.U):
            words = path_to_words(fast["paths"][u], graph["row_state"], n)
            assert [int(v) for v in la["labels"][u]] == words
            assert [int(v) for v in lgen["labels"][u]] == words
            np.testing.assert_array_equal(lc["labels_flat"][lc["label_off"][u]:lc["label_off"][u] + lc["n_labels"][u]], la["labels"][u])
        b.close()
    lat.close()
    gmm.close()


def test_bigram_kernel_breaks_ties_like_the_reference(hip, ctx):
    """Small-integer transition and bigram costs over word models that come in identical PAIRS (words 2k and 2k+1 share
    their Gaussians), so that two predecessor words reach an entry row at exactly the same cost in nearly every column.
    The broadcasts deliver the candidates in ascending word order and the reduction keeps the left operand on a tie:
    the path must be the oracle's (np.argmin's first minimum) -- and the test counts, with the oracle's own cost
    matrices, the entry-row cells ON the decoded paths that really had two equal best predecessors."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(4242)
    W, n, M, D = 8, 3, 1, 4
    half = make_model(rng, W // 2, n, M, D)
    means, vars_, w = (np.repeat(a, 2, axis=0) for a in half)
    t1 = [word_trans(rng, n, integer=True) for _ in range(W // 2)]
    wt = [t1[i // 2] for i in range(W)]
    Bh = rng.integers(0, 4, size=(W // 2, W)).astype(np.float64)
    B = np.repeat(Bh, 2, axis=0)                                  # rows 2k and 2k+1 equal: the twins tie as predecessors
    init = np.repeat(rng.integers(0, 3, size=W // 2), 2).astype(np.float64)
    xs = make_utts(rng, means, vars_, 30, short_every=0)
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    lat = hip.Lattices(ctx, [graph])
    assert "bigram" in lat.forms()
    b = hip.Batch(ctx, xs)
    nll = b.loglik(gmm)
    r = lat.viterbi(b, want_path=True)
    with forced(GMMHMM_VITERBI="generic"):
        gen = lat.viterbi(b, want_path=True)
    dense = dense_of(graph)
    first = 1 + W * (n - 1)
    ends = np.asarray(graph["end_rows"])
    ties_on_path = 0
    for u in range(b.U):
        costs, path = oracle_decode(graph, nll[b.offsets[u]:b.offsets[u + 1]])
        np.testing.assert_array_equal(r["paths"][u], path)
        np.testing.assert_array_equal(gen["paths"][u], path)
        assert int(r["best_end"][u]) == oracle_best_end(costs, ends)
        np.testing.assert_allclose(r["end_cost"][u], costs[ends, -1], rtol=1e-10)
        for row, col in path:
            if first <= row < first + W:
                cand = dense[row] + costs[:, col]
                ties_on_path += int(np.sum(cand == cand.min()) > 1)
    assert ties_on_path >= 10, ties_on_path
    b.close(); lat.close(); gmm.close()


def test_graphs_that_miss_the_layout_do_not_get_the_bit(hip, ctx):
    """17 words, and near misses of the layout (an entry row fed by a non-final state, a cost on entry row -> state 0, a
    missing entry arc, an entry row feeding another word, the two row blocks in the other order): no "bigram" bit, and the decode -- on the row-per-lane
    kernels -- still equals the oracle."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(17)
    n = 3
    cases = []
    W = 17
    B, init = random_costs(rng, W, 0.2)
    cases.append(("17 words", W, packed_bigram_lattice([word_trans(rng, n) for _ in range(W)], n, B, init)[0]))
    W = 4
    wt = [word_trans(rng, n) for _ in range(W)]
    B, init = random_costs(rng, W, 0.0)
    base = packed_bigram_lattice(wt, n, B, init)[0]
    assert "bigram" in hip.Lattices(ctx, [base]).forms()
    first = 1 + W * (n - 1)

    def variant(fn):
        g = {k: np.array(v) for k, v in base.items()}
        fn(g)
        return g

    def extra_arc(to, frm, cost):
        def fn(g):
            g["arc_to"] = np.append(g["arc_to"], to).astype(np.int32)
            g["arc_from"] = np.append(g["arc_from"], frm).astype(np.int32)
            g["arc_cost"] = np.append(g["arc_cost"], cost)
        return fn

    def entry_cost(g):
        k = np.flatnonzero((g["arc_from"] == first + 1) & (g["arc_to"] == first + W + 1))[0]
        g["arc_cost"][k] = 0.25

    def drop_entry(g):
        keep = ~((g["arc_from"] == first + 2) & (g["arc_to"] == first + W + 2))
        for k in ("arc_to", "arc_from", "arc_cost"):
            g[k] = g[k][keep]

    cases.append(("entry row fed by a non-final state", W, variant(extra_arc(first + 1, 1, 0.5))))      # row 1 = word 0, state 1
    cases.append(("cost on entry row -> state 0", W, variant(entry_cost)))
    cases.append(("missing entry arc", W, variant(drop_entry)))
    cases.append(("entry row feeding another word", W, variant(extra_arc(first + W + 3, first, 0.0))))

    def swap_blocks(g):                                       # state-0 rows in front of the entry rows
        perm = np.arange(len(g["row_state"]))
        perm[first:first + W], perm[first + W:first + 2 * W] = np.arange(first + W, first + 2 * W), np.arange(first, first + W)
        rs = g["row_state"].copy()
        g["row_state"][perm] = rs
        for k in ("arc_to", "arc_from", "end_rows"):
            g[k] = perm[g[k]].astype(np.int32)

    cases.append(("rows out of order", W, variant(swap_blocks)))
    for name, W, graph in cases:
        means, vars_, w = make_model(rng, W, n)
        M, D = means.shape[2:]
        gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
        lat = hip.Lattices(ctx, [graph])
        assert "bigram" not in lat.forms(), name
        b = hip.Batch(ctx, make_utts(rng, means, vars_, 9, short_every=0, max_words=3))
        nll = b.loglik(gmm)
        r = lat.viterbi(b, want_path=True)
        check_against_oracle(graph, r, nll, b.offsets, rtol=1e-10)
        b.close(); lat.close(); gmm.close()


def test_constant_bigram_equals_loop_kernel(hip, ctx):
    """B = p everywhere, init = 0: the bigram-form kernel's end costs are BIT-EQUAL to the loop-form kernel's on
    packed_loop_lattice(word_penalty = p), best ends and word strings the same."""
    from sr.recognition.continuous_speech import packed_bigram_lattice, packed_loop_lattice
    for W, n, skip, p in ((10, 5, False, 2.5), (16, 3, True, 0.0), (3, 8, False, 1.0)):
        rng = np.random.default_rng(31 * W + n)
        means, vars_, w = make_model(rng, W, n)
        M, D = means.shape[2:]
        wt = [word_trans(rng, n, skip) for _ in range(W)]
        gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
        gb = packed_bigram_lattice(wt, n, np.full((W, W), p))[0]
        gl = packed_loop_lattice(wt, n, p)[0]
        lb, ll = hip.Lattices(ctx, [gb]), hip.Lattices(ctx, [gl])
        assert "bigram" in lb.forms() and "loop" in ll.forms()
        b = hip.Batch(ctx, make_utts(rng, means, vars_, 37))
        b.loglik(gmm, fetch=False)
        rb, rl = lb.viterbi(b, want_path=False), ll.viterbi(b, want_path=False)
        np.testing.assert_array_equal(rb["end_cost_flat"], rl["end_cost_flat"])
        np.testing.assert_array_equal(rb["best_end"], rl["best_end"])
        wb = lb.viterbi_labels(b, np.where(gb["row_state"] >= 0, gb["row_state"] // n, -1).astype(np.int32))
        wl = ll.viterbi_labels(b, np.where(gl["row_state"] >= 0, gl["row_state"] // n, -1).astype(np.int32))
        for u in range(b.U):
            np.testing.assert_array_equal(wb["labels"][u], wl["labels"][u])
        b.close(); lb.close(); ll.close(); gmm.close()


def test_bigram_decodes_in_three_or_more_chunks(hip, ctx):
    """A small GMMHMM_SCRATCH_BUDGET cuts the decode into >= 3 launches: paths and on-device labels equal the one-launch
    run bit for bit."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(12)
    W, n = 6, 4
    means, vars_, w = make_model(rng, W, n)
    M, D = means.shape[2:]
    wt = [word_trans(rng, n) for _ in range(W)]
    B, init = random_costs(rng, W, 0.2)
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    lat = hip.Lattices(ctx, [graph])
    assert "bigram" in lat.forms()
    b = hip.Batch(ctx, make_utts(rng, means, vars_, 48))
    b.loglik(gmm, fetch=False)
    row_word = np.where(graph["row_state"] >= 0, graph["row_state"] // n, -1).astype(np.int32)
    one_p = lat.viterbi(b, want_path=True)
    assert ctx.last_chunks == 1
    one_l = lat.viterbi_labels(b, row_word, as_lists=False)
    with forced(GMMHMM_SCRATCH_BUDGET="4K"):      # decision words: 64 B per 3 columns and utterance
        many_p = lat.viterbi(b, want_path=True)
        assert ctx.last_chunks >= 3, ctx.last_chunks
        many_l = lat.viterbi_labels(b, row_word, as_lists=False)
        assert ctx.last_chunks >= 3, ctx.last_chunks
    np.testing.assert_array_equal(one_p["end_cost_flat"], many_p["end_cost_flat"])
    np.testing.assert_array_equal(one_p["best_end"], many_p["best_end"])
    for x, y in zip(one_p["paths"], many_p["paths"]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(one_l["n_labels"], many_l["n_labels"])
    for u in range(b.U):
        np.testing.assert_array_equal(one_l["labels_flat"][one_l["label_off"][u]:one_l["label_off"][u] + one_l["n_labels"][u]],
                                      many_l["labels_flat"][many_l["label_off"][u]:many_l["label_off"][u] + many_l["n_labels"][u]])
    b.close(); lat.close(); gmm.close()


def test_bigram_rank_beam_equals_oracle(hip, ctx):
    """A rank beam sends the bigram graph to the generic kernel like every other form: cells and paths equal the oracle's
    lattice beam; a beam of all rows is the unpruned decode bit for bit."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(43)
    W, n = 5, 3
    means, vars_, w = make_model(rng, W, n)
    M, D = means.shape[2:]
    wt = [word_trans(rng, n) for _ in range(W)]
    B, init = random_costs(rng, W, 0.15)
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    R = len(graph["row_state"])
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    lat = hip.Lattices(ctx, [graph])
    b = hip.Batch(ctx, make_utts(rng, means, vars_, 10, short_every=0, max_words=3))
    nll = b.loglik(gmm)
    base = lat.viterbi(b, want_path=True)
    ends = np.asarray(graph["end_rows"])
    for beam in (5, 11, R):
        lat.set_beam(beam)
        r = lat.viterbi(b, want_path=True, want_costs=True)
        compared = 0
        for u in range(b.U):
            try:
                costs, path = oracle_decode(graph, nll[b.offsets[u]:b.offsets[u + 1]], beam=beam)
            except RuntimeError:
                continue                                      # every end pruned away: the reference-style walk does not terminate
            fin = np.isfinite(costs)
            np.testing.assert_array_equal(np.isfinite(r["costs"][u]), fin)
            np.testing.assert_allclose(r["costs"][u][fin], costs[fin], rtol=1e-12)
            if np.isfinite(costs[ends, -1]).any():
                np.testing.assert_array_equal(r["paths"][u], path)
                compared += 1
        assert compared > 0
        if beam == R:
            np.testing.assert_array_equal(r["end_cost_flat"], base["end_cost_flat"])
            for u in range(b.U):
                np.testing.assert_array_equal(r["paths"][u], base["paths"][u])
    lat.set_beam(None)
    b.close(); lat.close(); gmm.close()


def _toy_models(rng, W, n, D, M=2):
    """(HMM objects, means [W, n, M, D], variances [W, n, M, D])"""
    from sr.recognition.hmm import HMM
    from sr.recognition.hmm_state import GMM
    means = rng.normal(size=(W, n, M, D)) * 3.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    models = []
    for i in range(W):
        h = HMM(n)
        h.gmm_states = []
        for s in range(n):
            g = GMM(means[i, s, 0].copy(), vars_[i, s, 0].copy(), M)
            g.update_models(means[i, s].copy(), vars_[i, s].copy(), rng.dirichlet(np.ones(M)))
            h.gmm_states.append(g)
        h.transitions = word_trans(rng, n)
        h.mu, h.sigma = means[i, :, 0].copy(), vars_[i, :, 0].copy()
        models.append(h)
    return models, means, vars_


def test_continuous_decoder_bigram_end_to_end(hip, ctx):
    """ContinuousDecoder(grammar="bigram"), from cost arrays and from a fitted BigramModel: the word strings equal the
    oracle's decode of build_bigram_grammar's graph on the same likelihoods; want_path=True and False agree; accuracy
    tallies; the other grammars' arguments are unchanged."""
    from sr.langmodel import BigramModel
    from sr.recognition.batch import ContinuousDecoder
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(8)
    W, n, D = 4, 3, 5
    models, mm, vv = _toy_models(rng, W, n, D)
    corpus = [[0, 1, 2], [1, 2, 3], [0, 1], [2, 3, 0, 1]]
    lm = BigramModel(W, smoothing=0).fit(corpus)               # unseen pairs are forbidden
    xs = make_utts(rng, mm, vv, 12, short_every=0, max_words=4)
    init, B = lm.costs()
    for kwargs in (dict(bigram=lm), dict(bigram=B, initial=init), dict(bigram=lm, lm_scale=2.0)):
        dec = ContinuousDecoder(models, grammar="bigram", ctx=ctx, **kwargs)
        assert "bigram" in dec.lat.forms()
        scale = kwargs.get("lm_scale", 1.0)
        graph = packed_bigram_lattice([m.transitions for m in models], n, B * scale, init * scale)[0]
        batch = hip.Batch(ctx, xs)
        words_l, _ = dec.decode_batch(batch, want_path=False)
        words_p, rp = dec.decode_batch(batch, want_path=True)
        nll = batch.loglik(dec.gmm)
        assert words_l == words_p
        nes = graph["row_state"] < 0
        rw = np.where(nes, -1, graph["row_state"] // n)
        for u in range(len(xs)):
            costs, path = oracle_decode(graph, nll[batch.offsets[u]:batch.offsets[u + 1]])
            np.testing.assert_array_equal(rp["paths"][u], path)
            assert words_l[u] == O.path_to_words(path, nes, rw)
            assert all(np.isfinite(B[a, c]) for a, c in zip(words_l[u][:-1], words_l[u][1:]))
        assert dec.decode(xs) == words_l
        rep = dec.accuracy(xs, words_l)
        assert rep["sequence_accuracy"] == 1.0
        batch.close()
    with pytest.raises(ValueError):
        ContinuousDecoder(models, grammar="bigram", ctx=ctx)
    with pytest.raises(ValueError):
        ContinuousDecoder(models, grammar="bigram", ctx=ctx, bigram=np.zeros((W, W + 1)))
    with pytest.raises(ValueError):
        ContinuousDecoder(models, grammar="bigram", ctx=ctx, bigram=BigramModel(W + 1).fit([[0]]))
    with pytest.raises(ValueError):
        ContinuousDecoder(models, grammar="trigram", ctx=ctx)


def test_continuous_decoder_bigram_beyond_the_form(hip, ctx):
    """17 words: no form bit, the decoder still decodes (row-per-lane kernels) and equals the oracle."""
    from sr.recognition.batch import ContinuousDecoder
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(9)
    W, n, D = 17, 2, 4
    models, mm, vv = _toy_models(rng, W, n, D)
    B, init = random_costs(rng, W, 0.2)
    dec = ContinuousDecoder(models, grammar="bigram", ctx=ctx, bigram=B, initial=init)
    assert "bigram" not in dec.lat.forms()
    xs = make_utts(rng, mm, vv, 6, short_every=0, max_words=3)
    batch = hip.Batch(ctx, xs)
    words, _ = dec.decode_batch(batch)
    nll = batch.loglik(dec.gmm)
    graph = packed_bigram_lattice([m.transitions for m in models], n, B, init)[0]
    nes = graph["row_state"] < 0
    rw = np.where(nes, -1, graph["row_state"] // n)
    for u in range(len(xs)):
        _, path = oracle_decode(graph, nll[batch.offsets[u]:batch.offsets[u + 1]])
        assert words[u] == O.path_to_words(path, nes, rw)
    batch.close()
