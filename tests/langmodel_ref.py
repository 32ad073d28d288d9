# -*- coding: utf-8 -*-
"""Numpy restatement of text_viterbi (sr/langmodel/spellchecker.py) for the tests: the recurrence of
csrc/gh_lextree.hip, column by column, the insertion chain one depth level at a time, integer costs.  Test-only."""
import numpy as np

INF = np.iinfo(np.int64).max // 4


def encode(x, flat, dist_fun):
    """Per-column distance rows [C, R] of '*' + x against the flattened tree's values."""
    xs = "*" + x
    cache = {}
    d = np.empty((len(xs), flat.R), dtype=np.int64)
    for c, ch in enumerate(xs):
        if ch not in cache:
            cache[ch] = np.array([int(dist_fun(ch, v)) for v in flat.vals], dtype=np.int64)
        d[c] = cache[ch]
    return d


def text_viterbi_rows(d, parent, depth, word_ends):
    """(best cost, back-trace rows) for distance rows d [C, R]; parent / depth / word_ends as FlatTree has them."""
    C, R = d.shape
    assert C >= 2
    sp = R - 1
    we = np.asarray(word_ends)
    tree_rows = np.arange(1, R - 1)
    levels = [tree_rows[depth[1:R - 1] == L] for L in range(1, int(depth.max()) + 1)]
    par = parent.astype(np.int64)
    has_match = np.zeros(R, dtype=bool)
    has_match[tree_rows] = par[tree_rows] != 0
    dec = np.zeros((C, R), dtype=np.int8)
    arg = np.zeros((C, 2), dtype=np.int64)
    prev = None
    for c in range(C):
        cur = np.full(R, INF, dtype=np.int64)
        if c == 0:
            cur[0] = 0
            cur[sp] = d[0, sp] if 0 in we[1:] else INF   # (the root as a word end: its initial 0 in the wrapped column)
            best = np.full(R, INF, dtype=np.int64)
        else:
            v = prev[we]
            k_all = int(np.argmin(v))
            k_sp = 1 + int(np.argmin(v[1:]))
            arg[c] = (k_all, k_sp)
            cur[0] = d[c, 0] + 1 + v[k_all]
            cur[sp] = d[c, sp] + v[k_sp]
            dele = d[c] + 1 + prev
            match = np.where(has_match, d[c] + prev[np.maximum(par, 0)], INF)
            best = np.minimum(dele, match)
            dec[c] = np.where(match < dele, 1, 0)
        for rows in levels:
            ins = d[c, rows] + 1 + cur[par[rows]]
            take = ins < best[rows]
            best[rows] = np.where(take, ins, best[rows])
            dec[c, rows] = np.where(take, 2, dec[c, rows])
            cur[rows] = best[rows]
        prev = cur
    k = int(np.argmin(prev[we]))
    r, c = int(we[k]), C - 1
    rows = [r]
    while c != 1:
        if r == 0:
            r, c = int(we[arg[c, 0]]), c - 1
        elif r == sp:
            r, c = int(we[arg[c, 1]]), c - 1
        else:
            dd = dec[c, r]
            if dd != 0:
                r = int(par[r])
            if dd != 2:
                c -= 1
        if r != 0:
            rows.append(r)
    return int(prev[we[k]]), rows


def text_viterbi(x, flat, dist_fun=lambda a, b: int(a != b)):
    """(cost as np.float64, matched string), as the reference returns them."""
    cost, rows = text_viterbi_rows(encode(x, flat, dist_fun), flat.parent, flat.depth, flat.word_ends)
    s = flat.vals[rows[0]]
    for r in rows[1:]:
        s += flat.vals[r]
    return np.float64(cost), s[::-1]
