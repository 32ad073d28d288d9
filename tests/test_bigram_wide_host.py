# -*- coding: utf-8 -*-
"""The wide bigram form (17 to 64 words) on the host, no GPU.

1. `_hip.Lattices.FORMS` names the seven form bits of `gh_lattices_forms` in order; the header documents bit 6.
2. `packed_bigram_lattice` at 64 words has the row layout the recogniser of csrc/gh_lattice.hip documents.
3. The oracle's decode of a 20-word bigram graph equals a brute-force restatement of the min-plus recursion: the
   candidate order (ascending predecessor word, first minimum) that gh_viterbi_bigram_wide.hip is written against."""
import os
import re
import warnings

import numpy as np

from conftest import ROOT
from oracle import ref_numpy as O


def word_trans(rng, n, skip=False, integer=False):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = (float(rng.integers(0, 2)) if integer else rng.uniform(0.05, 0.6)) if i < n - 1 else 0.0
        if i < n - 1:
            t[i + 1, i] = float(rng.integers(1, 3)) if integer else rng.uniform(0.8, 2.5)
        if skip and i < n - 2 and rng.random() < 0.6:
            t[i + 2, i] = float(rng.integers(2, 4)) if integer else rng.uniform(1.5, 4.0)
    return t


def test_forms_names_the_seven_bits_in_order():
    from sr.recognition import _hip
    assert _hip.Lattices.FORMS == ("chain", "layers", "loop", "sequence", "fb_chain", "bigram", "bigram_wide")
    header = open(os.path.join(ROOT, "include", "gmmhmm.h")).read()
    doc = header[header.index("gh_lattices_forms") - 3000:header.index("gh_lattices_forms")]
    assert re.search(r"bit 6 \(64\)", doc), "include/gmmhmm.h does not document form bit 6"


def test_packed_bigram_lattice_has_the_documented_rows_at_64_words():
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(64)
    W, n = 64, 3
    B = rng.uniform(0.0, 4.0, size=(W, W))
    B[rng.random((W, W)) < 0.2] = np.inf
    init = rng.uniform(0.0, 2.0, size=W)
    g, nes_rows = packed_bigram_lattice([word_trans(rng, n) for _ in range(W)], n, B, init)
    rs = g["row_state"]
    R = 1 + W * (n - 1) + 2 * W
    first = 1 + W * (n - 1)
    assert len(rs) == R
    assert rs[0] < 0 and (rs[1:first] >= 0).all()                         # start row, states 1 .. n-1 of every word
    assert (rs[first:first + W] < 0).all()                                # W entry rows ...
    assert (rs[first + W:] >= 0).all()                                    # ... in front of the W state-0 rows
    assert nes_rows == [0] + list(range(first, first + W))
    for w in range(W):
        assert rs[first + W + w] == w * n
        assert list(rs[1 + w * (n - 1):1 + (w + 1) * (n - 1)]) == [w * n + s for s in range(1, n)]
    to, frm, cost = g["arc_to"], g["arc_from"], g["arc_cost"]
    for w in range(W):
        k = np.flatnonzero((to == first + W + w) & (frm == first + w))
        assert len(k) == 1 and cost[k[0]] == 0.0                          # entry row -> state 0 at cost 0
        into = np.flatnonzero(to == first + w)                            # last state of v -> entry row of w: B[v, w]
        v = (frm[into] - 1) // (n - 1)
        assert ((frm[into] - 1) % (n - 1) == n - 2).all()
        np.testing.assert_array_equal(np.sort(v), np.flatnonzero(np.isfinite(B[:, w])))
        np.testing.assert_array_equal(cost[into], B[v, w])
    assert list(g["end_rows"]) == [1 + w * (n - 1) + n - 2 for w in range(W)]      # emitting end rows: the words' last states
    assert not np.isnan(cost).any() and not ((to == frm) & (rs[to] < 0)).any()      # no NaN, no same-column self arc


def brute_force(E, wt, B, init):
    """The min-plus recursion of the bigram grammar, word by word (E [W, n, T]): (last-state costs of the last column,
    decoded words).  Candidates in ascending origin ROW order with a strict '<': inside a word the lower state first; into
    state 0 the start row (row 0), the entry row, then the state itself; into an entry row the lowest predecessor word."""
    W, n, T = E.shape
    prev = np.full((W, n), np.inf)
    back = []                                                 # per column: (in-word choice [W, n], entry arg [W], state-0 pick [W])
    for t in range(T):
        cur = np.full((W, n), np.inf)
        ch = np.zeros((W, n), dtype=int)
        for w in range(W):
            for s in range(1, n):
                best, arg = np.inf, -1
                for d in (2, 1, 0):                           # origins s-2, s-1, s
                    if s - d < 0 or np.isinf(wt[w][s, s - d]):
                        continue
                    c = prev[w, s - d] + wt[w][s, s - d]
                    if arg < 0 or c < best:
                        best, arg = c, d
                cur[w, s] = min(best + E[w, s, t], np.inf)
                ch[w, s] = arg
        earg = np.zeros(W, dtype=int)
        pick = np.zeros(W, dtype=int)
        for w in range(W):
            best, arg = np.inf, -1
            for v in range(W):
                if np.isinf(B[v, w]):
                    continue
                c = cur[v, n - 1] + B[v, w]
                if arg < 0 or c < best:
                    best, arg = c, v
            earg[w] = arg
            cands = []                                        # (cost, kind): 2 start row, 1 entry row, 0 self
            if not np.isinf(init[w]):
                cands.append(((0.0 if t == 0 else np.inf) + init[w], 2))
            cands.append((best, 1))
            if not np.isinf(wt[w][0, 0]):
                cands.append((prev[w, 0] + wt[w][0, 0], 0))
            b0, k0 = cands[0]
            for c, k in cands[1:]:
                if c < b0:
                    b0, k0 = c, k
            cur[w, 0] = min(b0 + E[w, 0, t], np.inf)
            pick[w] = k0
        back.append((ch, earg, pick))
        prev = cur
    ends = prev[:, n - 1]
    w = int(np.flatnonzero(ends == ends.min())[-1])           # the last of equal end points
    s, t, words = n - 1, T - 1, [w]
    while t > 0:
        ch, earg, pick = back[t]
        if s > 0:
            s -= ch[w, s]
            t -= 1
        elif pick[w] == 0:
            t -= 1
        elif pick[w] == 1:
            w, s = int(earg[w]), n - 1
            words.append(w)
        else:
            raise AssertionError("the start row in a column > 0")
    return ends, words[::-1]


def test_oracle_equals_the_brute_force_min_plus_recursion_at_20_words():
    from sr.recognition.continuous_speech import packed_bigram_lattice
    W, n = 20, 3
    for seed, integer in ((1, False), (2, False), (3, True), (4, True)):
        rng = np.random.default_rng(2000 + seed)
        wt = [word_trans(rng, n, skip=bool(seed % 2), integer=integer) for _ in range(W)]
        if integer:
            B = rng.integers(0, 3, size=(W, W)).astype(np.float64)
            init = rng.integers(0, 2, size=W).astype(np.float64)
        else:
            B = rng.uniform(0.0, 4.0, size=(W, W))
            init = rng.uniform(0.0, 2.0, size=W)
        B[rng.random((W, W)) < 0.2] = np.inf
        B[rng.integers(0, W, size=W), np.arange(W)] = 1.0     # every word keeps a way in
        T = 16
        E = rng.integers(0, 4, size=(W, n, T)).astype(np.float64) if integer else rng.uniform(0.5, 9.0, size=(W, n, T))
        for k, wd in enumerate(rng.integers(0, W, size=4)):   # a few cheap words, so that paths change word
            E[wd, :, 4 * k:4 * k + 4] *= 0.1
        g = packed_bigram_lattice(wt, n, B, init)[0]
        R = len(g["row_state"])
        dense = np.full((R, R), np.inf)
        dense[g["arc_to"], g["arc_from"]] = g["arc_cost"]
        nes = g["row_state"] < 0
        Er = np.zeros((R, T))
        Er[~nes] = E.reshape(W * n, T)[g["row_state"][~nes]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            costs, path = O.decode_states(Er, nes, dense, end_points=[[int(e), -1] for e in g["end_rows"]])
        ends, words = brute_force(E, wt, B, init)
        np.testing.assert_array_equal(costs[np.asarray(g["end_rows"]), -1], ends)
        rw = np.where(nes, -1, g["row_state"] // n)
        assert O.path_to_words(path, nes, rw) == words, seed
        assert len(set(words)) >= 2
