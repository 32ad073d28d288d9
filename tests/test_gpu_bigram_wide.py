# -*- coding: utf-8 -*-
"""The WIDE bigram-form kernel (gh_viterbi_bigram_wide.hip: 17 to 64 words, a wave per utterance, lane = word, the entry
rows as a 64 x 64 min-plus step over v_readlane scalars and an LDS image of the costs, 6-bit predecessor words in the
decision records) against the oracle, the generic kernel and the wide loop kernel.

`Lattices.viterbi(batch)` with ONE graph for the whole batch takes the kernel when the graph carries the "bigram_wide"
form bit; GMMHMM_VITERBI=generic keeps it out.  The helpers are those of test_gpu_bigram.py, copied."""
import contextlib
import os
import warnings

import numpy as np
import pytest

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
    """B [W, W] with a fraction `forbid` of +inf entries -- but every word keeps at least one way in -- and start costs
    with some +inf, at least one word finite."""
    B = rng.uniform(0.0, 4.0, size=(W, W))
    B[rng.random((W, W)) < forbid] = np.inf
    keep = rng.integers(0, W, size=W)
    B[keep, np.arange(W)] = rng.uniform(0.0, 4.0, size=W)
    init = rng.uniform(0.0, 2.0, size=W)
    init[rng.random(W) < 0.3] = np.inf
    init[int(rng.integers(0, W))] = rng.uniform(0.0, 2.0)
    return B, init


def make_model(rng, W, n, M=2, D=5):
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    return means, vars_, w


def make_utts(rng, means, vars_, U, short_every=5, max_words=3, words=None):
    """U utterances of 1 .. max_words random words (`words`: these word sequences instead), every `short_every`-th one
    shorter than any word."""
    W, n, M, D = means.shape
    xs = []
    for u in range(U):
        if short_every and u % short_every == short_every - 1:
            xs.append(rng.normal(size=(int(rng.integers(2, max(3, n))), D)) * 2.0)      # shorter than any word
            continue
        segs = []
        seq = words[u % len(words)] if words is not None else rng.integers(0, W, size=rng.integers(1, max_words + 1))
        for wd in seq:
            Tw = int(rng.integers(n, 2 * n + 3))
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


def oracle_decode(graph, nll_u, dense=None):
    nes = graph["row_state"] < 0
    E = np.zeros((len(nes), len(nll_u)))
    E[~nes] = nll_u[:, graph["row_state"][~nes]].T
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O.decode_states(E, nes, dense_of(graph) if dense is None else dense, end_points=[[int(e), -1] for e in graph["end_rows"]])


def oracle_best_end(costs, ends):
    ec = costs[np.asarray(ends), -1]
    return int(np.flatnonzero(ec == ec.min())[-1])           # the last of equal minima (decode.py:129-134)


def check_against_oracle(graph, r, nll, offsets, rtol, paths=True):
    """end costs (finite masks equal, values to rtol), best ends and paths against the oracle; returns the oracle's
    (costs, path) per utterance"""
    ends = np.asarray(graph["end_rows"])
    dense = dense_of(graph)
    out = []
    for u in range(len(offsets) - 1):
        costs, path = oracle_decode(graph, nll[offsets[u]:offsets[u + 1]], dense)
        ec = costs[ends, -1]
        fin = np.isfinite(ec)
        np.testing.assert_array_equal(np.isfinite(r["end_cost"][u]), fin)
        np.testing.assert_allclose(r["end_cost"][u][fin], ec[fin], rtol=rtol)
        if paths:
            assert int(r["best_end"][u]) == oracle_best_end(costs, ends)
            np.testing.assert_array_equal(r["paths"][u], path)
        out.append((costs, path))
    return out


def entry_hops(graph, W, n, path):
    """predecessor words of the entry-row cells on a path (end -> start order): the cell in front of an entry row"""
    first = 1 + W * (n - 1)
    hops = []
    for k in range(len(path) - 1):
        if first <= path[k][0] < first + W:
            hops.append((int(path[k + 1][0]) - 1) // (n - 1))
    return hops


def packed(hip, ctx, means, vars_, w):
    W, n, M, D = means.shape
    return hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))


# ----------------------------------------------------------------------------------------------------------------------
# 1. form bits
def test_form_bits(hip, ctx):
    """17, 33 and 64 words of 2 .. 8 states carry "bigram_wide" and not "bigram"; 16 words "bigram" only; 65 words and
    17 words of 12 states neither."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(1)

    def forms(W, n, skip=False):
        B, init = random_costs(rng, W, 0.2)
        lat = hip.Lattices(ctx, [packed_bigram_lattice([word_trans(rng, n, skip) for _ in range(W)], n, B, init)[0]])
        f = lat.forms()
        lat.close()
        return f

    for W in (17, 33, 64):
        for n in range(2, 9):
            for skip in (False, True):
                f = forms(W, n, skip)
                assert "bigram_wide" in f and "bigram" not in f, (W, n, skip, f)
    assert forms(16, 3) & {"bigram", "bigram_wide"} == {"bigram"}
    assert not forms(65, 3) & {"bigram", "bigram_wide"}
    assert not forms(17, 12) & {"bigram", "bigram_wide"}


def test_graphs_that_miss_the_layout_do_not_get_the_bit(hip, ctx):
    """Near misses of the layout at 20 words (an entry row fed by a non-final state, a cost on entry row -> state 0, a
    missing entry arc, an entry row feeding another word, the two row blocks in the other order): no bigram bit, and the
    decode -- on the row-per-lane kernels -- still equals the oracle."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(20)
    W, n = 20, 3
    wt = [word_trans(rng, n) for _ in range(W)]
    B, init = random_costs(rng, W, 0.0)
    base = packed_bigram_lattice(wt, n, B, init)[0]
    lat = hip.Lattices(ctx, [base])
    assert "bigram_wide" in lat.forms()
    lat.close()
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
        k = np.flatnonzero((g["arc_from"] == first + 17) & (g["arc_to"] == first + W + 17))[0]
        g["arc_cost"][k] = 0.25

    def drop_entry(g):
        keep = ~((g["arc_from"] == first + 18) & (g["arc_to"] == first + W + 18))
        for k in ("arc_to", "arc_from", "arc_cost"):
            g[k] = g[k][keep]

    def swap_blocks(g):                                       # state-0 rows in front of the entry rows
        perm = np.arange(len(g["row_state"]))
        perm[first:first + W], perm[first + W:first + 2 * W] = np.arange(first + W, first + 2 * W), np.arange(first, first + W)
        rs = g["row_state"].copy()
        g["row_state"][perm] = rs
        for k in ("arc_to", "arc_from", "end_rows"):
            g[k] = perm[g[k]].astype(np.int32)

    cases = [("entry row fed by a non-final state", variant(extra_arc(first + 17, 1, 0.5))),        # row 1 = word 0, state 1
             ("cost on entry row -> state 0", variant(entry_cost)),
             ("missing entry arc", variant(drop_entry)),
             ("entry row feeding another word", variant(extra_arc(first + W + 19, first, 0.0))),
             ("rows out of order", variant(swap_blocks))]
    means, vars_, w = make_model(rng, W, n)
    gmm = packed(hip, ctx, means, vars_, w)
    b = hip.Batch(ctx, make_utts(rng, means, vars_, 6, short_every=0))
    nll = b.loglik(gmm)
    for name, graph in cases:
        lat = hip.Lattices(ctx, [graph])
        assert not lat.forms() & {"bigram", "bigram_wide"}, name
        r = lat.viterbi(b, want_path=True)
        check_against_oracle(graph, r, nll, b.offsets, rtol=1e-10)
        lat.close()
    b.close(); gmm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 2. + 3. against the oracle and against the row-per-lane route
# word sequences whose hops leave words of every quarter of a 64-word wave (words >= W are folded back by the test)
SEQS64 = [[20, 5, 40], [55, 3, 18], [33, 60], [47, 62, 9], [2, 29, 51], [63, 31], [16, 48, 32]]


@pytest.mark.parametrize("n,skip", [(n, s) for n in range(2, 9) for s in (False, True) if n > 2 or not s])
def test_wide_kernel_equals_oracle_and_generic_kernel(hip, ctx, n, skip):
    """Every word size x skip arcs at 17, 33 and 64 words, both likelihood dtypes, 20 % forbidden pairs, utterances of up
    to three words and some shorter than one word.  Against the oracle on the kernel's own likelihoods: finite masks equal,
    end costs to 1e-10, best ends and paths exact.  Against GMMHMM_VITERBI=generic: end costs BITWISE, ends and paths equal.
    At 64 words the oracle's paths must hop out of a word of every 16-lane quarter above the first."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    for W in (17, 33, 64):
        rng = np.random.default_rng(100 * W + 10 * n + skip)
        means, vars_, w = make_model(rng, W, n, D=4 + (n + W) % 3)
        wt = [word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)]
        B, init = random_costs(rng, W, 0.2)
        seqs = [[wd % W for wd in s] for s in SEQS64]
        for s in seqs:                                        # the planted sequences are allowed
            init[s[0]] = min(init[s[0]], 1.0)
            for a, c in zip(s[:-1], s[1:]):
                B[a, c] = min(B[a, c], 1.0)
        xs = make_utts(rng, means, vars_, 9, short_every=5, words=seqs)
        gmm = packed(hip, ctx, means, vars_, w)
        graph = packed_bigram_lattice(wt, n, B, init)[0]
        lat = hip.Lattices(ctx, [graph])
        assert "bigram_wide" in lat.forms()
        for dtype in (np.float64, np.float32):
            b = hip.Batch(ctx, xs, dtype=dtype)
            nll = np.asarray(b.loglik(gmm), dtype=np.float64)
            fast = lat.viterbi(b, want_path=True)
            with forced(GMMHMM_VITERBI="generic"):
                gen = lat.viterbi(b, want_path=True)
            np.testing.assert_array_equal(fast["end_cost_flat"], gen["end_cost_flat"])
            np.testing.assert_array_equal(fast["best_end"], gen["best_end"])
            for u in range(b.U):
                np.testing.assert_array_equal(fast["paths"][u], gen["paths"][u])
            ref = check_against_oracle(graph, fast, nll, b.offsets, rtol=1e-10)
            nopath = lat.viterbi(b, want_path=False)
            np.testing.assert_array_equal(nopath["end_cost_flat"], fast["end_cost_flat"])
            np.testing.assert_array_equal(nopath["best_end"], fast["best_end"])
            if W == 64:                                       # the inputs reach the new ground
                hops = [v for _, path in ref for v in entry_hops(graph, W, n, path)]
                for lo in (16, 32, 48):
                    assert any(lo <= v < lo + 16 for v in hops), (lo, sorted(hops))
            b.close()
        lat.close()
        gmm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. ties
def test_wide_kernel_breaks_ties_like_the_reference(hip, ctx):
    """Small-integer transition and bigram costs over word models that come in identical PAIRS (words 2k and 2k+1 share
    their Gaussians and their rows of B): two predecessor words reach an entry row at exactly the same cost.  The scan
    takes the candidates in ascending word order under a strict '<': the path must be the oracle's (np.argmin's first
    minimum).  From the oracle's own cost matrices: some entry-row cell ON a decoded path had two or more equal minimal
    candidates with the lowest of them at word >= 16."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(4243)
    W, n, M, D = 40, 3, 1, 4
    half = make_model(rng, W // 2, n, M, D)
    means, vars_, w = (np.repeat(a, 2, axis=0) for a in half)
    t1 = [word_trans(rng, n, integer=True) for _ in range(W // 2)]
    wt = [t1[i // 2] for i in range(W)]
    Bh = rng.integers(0, 4, size=(W // 2, W)).astype(np.float64)
    B = np.repeat(Bh, 2, axis=0)                                  # rows 2k and 2k+1 equal: the twins tie as predecessors
    init = np.repeat(rng.integers(0, 3, size=W // 2), 2).astype(np.float64)
    seqs = [[20, 5, 38], [31, 17, 24], [9, 36], [26, 33, 3], [18, 22, 28]]
    xs = make_utts(rng, means, vars_, 10, short_every=0, words=seqs)
    gmm = packed(hip, ctx, means, vars_, w)
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    lat = hip.Lattices(ctx, [graph])
    assert "bigram_wide" in lat.forms()
    b = hip.Batch(ctx, xs)
    nll = b.loglik(gmm)
    r = lat.viterbi(b, want_path=True)
    dense = dense_of(graph)
    first = 1 + W * (n - 1)
    ties_high = 0
    for u, (costs, path) in enumerate(check_against_oracle(graph, r, nll, b.offsets, rtol=1e-10)):
        for row, col in path:
            if first <= row < first + W:
                cand = dense[row] + costs[:, col]
                at = np.flatnonzero(cand == cand.min())
                ties_high += int(len(at) > 1 and np.isfinite(cand.min()) and (at[0] - 1) // (n - 1) >= 16)
    assert ties_high >= 1, ties_high
    b.close(); lat.close(); gmm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. constant B: the wide loop kernel
def test_constant_bigram_equals_wide_loop_kernel(hip, ctx):
    """B = p everywhere, init = 0: the wide bigram kernel's end costs are BIT-EQUAL to the wide loop kernel's on
    packed_loop_lattice(word_penalty = p), best ends and word strings the same."""
    from sr.recognition.continuous_speech import packed_bigram_lattice, packed_loop_lattice
    for W, n, skip, p in ((17, 5, False, 2.5), (40, 3, True, 0.0), (64, 8, False, 1.0)):
        rng = np.random.default_rng(31 * W + n)
        means, vars_, w = make_model(rng, W, n)
        wt = [word_trans(rng, n, skip) for _ in range(W)]
        gmm = packed(hip, ctx, means, vars_, w)
        gb = packed_bigram_lattice(wt, n, np.full((W, W), p))[0]
        gl = packed_loop_lattice(wt, n, p)[0]
        lb, ll = hip.Lattices(ctx, [gb]), hip.Lattices(ctx, [gl])
        assert "bigram_wide" in lb.forms() and "loop" in ll.forms()
        b = hip.Batch(ctx, make_utts(rng, means, vars_, 11))
        b.loglik(gmm, fetch=False)
        rb, rl = lb.viterbi(b, want_path=False), ll.viterbi(b, want_path=False)
        np.testing.assert_array_equal(rb["end_cost_flat"], rl["end_cost_flat"])
        np.testing.assert_array_equal(rb["best_end"], rl["best_end"])
        wb = lb.viterbi_labels(b, np.where(gb["row_state"] >= 0, gb["row_state"] // n, -1).astype(np.int32))
        wl = ll.viterbi_labels(b, np.where(gl["row_state"] >= 0, gl["row_state"] // n, -1).astype(np.int32))
        for u in range(b.U):
            np.testing.assert_array_equal(wb["labels"][u], wl["labels"][u])
        assert any(len(x) > 1 for x in wb["labels"])
        b.close(); lb.close(); ll.close(); gmm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 6. an entry row whose every candidate is +inf
def all_inf_entry_case(rng):
    """52 two-state words without a self arc on the last state (so that an unreachable last state has ONE origin, its
    word's state 0, and the walk over +inf cells is the same first-existing-arc walk in the reference and in the kernel).
    Word 7 can be entered from words 40 and 50 only; those two cannot start an utterance and follow nothing but each
    other, so their last states are +inf in every column -- and with them every candidate of word 7's entry row."""
    W, n = 52, 2
    means, vars_, w = make_model(rng, W, n)
    wt = [word_trans(rng, n, last_self=np.inf) for _ in range(W)]
    B, init = random_costs(rng, W, 0.2)
    B[:, 7] = np.inf
    B[40, 7], B[50, 7] = 0.5, 0.25
    B[:, 40] = np.inf
    B[:, 50] = np.inf
    B[50, 40], B[40, 50] = 1.0, 1.0
    init[[7, 40, 50]] = np.inf
    xs = make_utts(rng, means, vars_, 8, short_every=0, words=[[7, 3], [12, 7], [7], [45, 7, 7]])
    return W, n, means, vars_, w, wt, B, init, xs


def test_entry_row_with_only_infinite_candidates(hip, ctx):
    """The reference's back-trace leaves an entry row whose candidates are all +inf through its first EXISTING arc (word 40
    here); the sweep recorded word 0, which has no arc into that row, and the back-trace must put word 40 in its place
    from the 64-bit arc mask, without tripping its flag.  With every word's end: end costs, ends and paths equal the
    oracle's, word 7's end is +inf.  With word 7's end as the only end: the path is the walk over +inf cells through that
    entry row, equal to the oracle's, cell by cell."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    W, n, means, vars_, w, wt, B, init, xs = all_inf_entry_case(np.random.default_rng(66))
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    ends = np.asarray(graph["end_rows"])
    g7 = dict(graph, end_rows=np.array([ends[7]], dtype=np.int32))
    first = 1 + W * (n - 1)
    gmm = packed(hip, ctx, means, vars_, w)
    b = hip.Batch(ctx, xs)
    nll = b.loglik(gmm)
    for g in (graph, g7):
        lat = hip.Lattices(ctx, [g])
        assert "bigram_wide" in lat.forms()
        r = lat.viterbi(b, want_path=True)                    # (a tripped flag raises)
        ref = check_against_oracle(g, r, nll, b.offsets, rtol=1e-10)
        lat.close()
        if g is graph:
            for costs, _ in ref:
                assert np.isinf(costs[ends[7], -1]) and np.isinf(costs[first + 7]).all() and np.isfinite(costs[ends, -1]).any()
        else:
            through = 0
            for _, path in ref:
                rows = [int(p[0]) for p in path]
                for k in range(len(rows) - 1):
                    if rows[k] == first + 7:
                        assert rows[k + 1] == 1 + 40 * (n - 1) + n - 2          # the last state of word 40
                        through += 1
            assert through >= 4, "the oracle's paths do not stand on the all-inf entry row"
    b.close(); gmm.close()


# ----------------------------------------------------------------------------------------------------------------------
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


# 7. labels and times
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_labels_and_times(hip, ctx, dtype):
    """ContinuousDecoder(grammar="bigram") at 33 words: decode_batch words equal O.path_to_words of the oracle's path,
    want_times=True begins equal path_to_word_times of the same decode's path; slot and packed label layouts agree."""
    from sr.recognition.batch import ContinuousDecoder, path_to_word_times
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(77)
    W, n, D = 33, 4, 5
    models, mm, vv = _toy_models(rng, W, n, D)
    B, init = random_costs(rng, W, 0.2)
    dec = ContinuousDecoder(models, grammar="bigram", ctx=ctx, bigram=B, initial=init, dtype=dtype)
    assert "bigram_wide" in dec.lat.forms()
    xs = make_utts(rng, mm, vv, 10, short_every=5)
    batch = hip.Batch(ctx, xs, dtype=dtype)
    words, _ = dec.decode_batch(batch)
    words_t, rt = dec.decode_batch(batch, want_times=True)
    words_p, rp = dec.decode_batch(batch, want_path=True, want_times=True)
    nll = np.asarray(batch.loglik(dec.gmm), dtype=np.float64)
    graph = packed_bigram_lattice([m.transitions for m in models], n, B, init)[0]
    nes = graph["row_state"] < 0
    rw = np.where(nes, -1, graph["row_state"] // n)
    assert words == words_t == words_p
    for u in range(len(xs)):
        _, path = oracle_decode(graph, nll[batch.offsets[u]:batch.offsets[u + 1]])
        np.testing.assert_array_equal(rp["paths"][u], path)
        assert words[u] == O.path_to_words(path, nes, rw)
        wu, bu = path_to_word_times(rp["paths"][u], dec.row_state, n)
        assert wu == words[u]
        assert [int(v) for v in rt["begins"][u]] == [int(v) for v in bu] == [int(v) for v in rp["begins"][u]]
    assert any(len(x) > 1 for x in words)
    row_word = rw.astype(np.int32)
    for kw in (dict(), dict(want_begin=True)):
        slot = dec.lat.viterbi_labels(batch, row_word, **kw)                     # a slot of the path capacity per utterance
        pk = dec.lat.viterbi_labels(batch, row_word, as_lists=False, **kw)       # packed: only the labels that exist
        for u in range(len(xs)):
            k = int(slot["n_labels"][u])
            assert k == int(pk["n_labels"][u]) == len(words[u])
            c = pk["labels_flat"][pk["label_off"][u]:pk["label_off"][u] + k]
            assert list(slot["labels"][u]) == list(c) == words[u]
            if kw:
                bc = pk["begins_flat"][pk["label_off"][u]:pk["label_off"][u] + k]
                assert list(slot["begins"][u]) == list(bc) == [int(v) for v in rt["begins"][u]]
    batch.close()


# 8. chunks
def test_wide_bigram_decodes_in_three_or_more_chunks(hip, ctx):
    """A small GMMHMM_SCRATCH_BUDGET cuts the decode into >= 3 launches: ends, paths and on-device labels equal the
    one-launch run bit for bit."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(12)
    W, n = 24, 4
    means, vars_, w = make_model(rng, W, n)
    wt = [word_trans(rng, n) for _ in range(W)]
    B, init = random_costs(rng, W, 0.2)
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    gmm = packed(hip, ctx, means, vars_, w)
    lat = hip.Lattices(ctx, [graph])
    assert "bigram_wide" in lat.forms()
    b = hip.Batch(ctx, make_utts(rng, means, vars_, 12))
    b.loglik(gmm, fetch=False)
    row_word = np.where(graph["row_state"] >= 0, graph["row_state"] // n, -1).astype(np.int32)
    one_p = lat.viterbi(b, want_path=True)
    assert ctx.last_chunks == 1
    one_l = lat.viterbi_labels(b, row_word, as_lists=False)
    with forced(GMMHMM_SCRATCH_BUDGET="16K"):     # decision words: 256 B per column and utterance
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


# 9. a one-frame utterance in the batch
def test_batch_with_a_one_frame_utterance_falls_back(hip, ctx):
    """T == 1 has the reference's column wrap, which only the lean / generic kernels implement: the whole batch leaves the
    wide kernel and still equals the oracle."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(91)
    W, n = 19, 3
    means, vars_, w = make_model(rng, W, n)
    wt = [word_trans(rng, n) for _ in range(W)]
    B, init = random_costs(rng, W, 0.2)
    graph = packed_bigram_lattice(wt, n, B, init)[0]
    gmm = packed(hip, ctx, means, vars_, w)
    lat = hip.Lattices(ctx, [graph])
    assert "bigram_wide" in lat.forms()
    xs = make_utts(rng, means, vars_, 6, short_every=0)
    xs.insert(2, rng.normal(size=(1, means.shape[3])))
    b = hip.Batch(ctx, xs)
    nll = b.loglik(gmm)
    r = lat.viterbi(b, want_path=True)
    ends = np.asarray(graph["end_rows"])
    nes = graph["row_state"] < 0
    for u in range(b.U):
        nll_u = nll[b.offsets[u]:b.offsets[u + 1]]
        if len(nll_u) > 1:
            costs, path = oracle_decode(graph, nll_u)
        else:                                                 # one column: the fill alone (the reference's walk needs two)
            E = np.zeros((len(nes), 1))
            E[~nes] = nll_u[:, graph["row_state"][~nes]].T
            costs = O.decode_fill(E, nes, dense_of(graph))[0]
        ec = costs[ends, -1]
        fin = np.isfinite(ec)
        np.testing.assert_array_equal(np.isfinite(r["end_cost"][u]), fin)
        np.testing.assert_allclose(r["end_cost"][u][fin], ec[fin], rtol=1e-10)
        if len(nll_u) > 1:
            assert int(r["best_end"][u]) == oracle_best_end(costs, ends)
            np.testing.assert_array_equal(r["paths"][u], path)
    b.close(); lat.close(); gmm.close()


# 10. refusals
def test_online_and_word_stream_refusals_are_unchanged(hip, ctx):
    """Through the real library, on a 17-word bigram decoder: online_bigram, online and a word-stream session are refused
    with Unsupported (gh_online_create_bigram[_settle], gh_online_create*, gh_wordstream_create go by the narrow form's
    flag), before any kernel runs."""
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(10)
    W, n, D = 17, 3, 4
    models, mm, vv = _toy_models(rng, W, n, D)
    B, init = random_costs(rng, W, 0.2)
    dec = ContinuousDecoder(models, grammar="bigram", ctx=ctx, bigram=B, initial=init)
    assert "bigram_wide" in dec.lat.forms() and "bigram" not in dec.lat.forms()
    for kw in (dict(max_frames=50), dict(max_frames=50, settle=True), dict(window=20)):
        with pytest.raises(hip.Unsupported, match="not in bigram form"):
            dec.online_bigram(n_streams=2, **kw)
    with pytest.raises(hip.Unsupported):
        dec.online(n_streams=2, max_frames=50)
    for make in (lambda: hip.OnlineSession(ctx, dec.lat, 2, 50), lambda: hip.OnlineSession(ctx, dec.lat, 2, window=20),
                 lambda: hip.OnlineWideSession(ctx, dec.lat, 2, 50), lambda: hip.OnlineBigramSession(ctx, dec.lat, 2, 50),
                 lambda: hip.WordStreamSession(ctx, dec.lat, 2)):
        with pytest.raises(hip.Unsupported):
            make()
