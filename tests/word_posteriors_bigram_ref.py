# -*- coding: utf-8 -*-
"""Word posteriors of the bigram grammar on the host (test infrastructure, no GPU, no `sr` package).

Rows as `build_bigram_grammar` lays them out: start | states 1..n-1 of every word | W entry rows L_u | W state-0 rows.
Notation of `O.forward_backward`: log alpha la, log beta lb, log P, costs trans[to, from]; last_w the last state of word w,
B[w, u] = trans[L_u, last_w].  A path's WORD AT FRAME t is the word of the LAST emitting cell it visits in column t:

    q_t(w) = sum_s gamma_t(w, s)  -  sum_u exp( la[last_w, t] - B[w, u] + lb[L_u, t] - logP )

(the subtracted sum: leaving word w through any entry row in column t).

  `bigram_graph`            the dense graph from word transitions, B and the start costs
  `forward_backward`        `O.forward_backward`'s recursion in any dtype (np.longdouble); float64 goes to the oracle itself
  `q_from_matrices`         the formula on given la, lb, log P
  `word_posteriors_bigram`  the formula on `forward_backward`: THE restatement
  `sweep`                   the same recursion written per column over [W, n] arrays (what the device kernel does), in any
                            dtype: the restatement at sizes where a row-by-row recursion in Python takes minutes.  The host
                            tests hold it to `word_posteriors_bigram` at 1e-12.
`brute_force` and `confidence` come from tests/word_posteriors_ref.py: they take any graph with is_nes and row_word."""
import numpy as np

from oracle import ref_numpy as O
from word_posteriors_ref import brute_force, confidence  # noqa: F401  (re-exported)


def bigram_graph(word_trans, n, B, init):
    """(trans [R, R], is_nes [R], row_word [R], ends, entry [W], row_of [W, n]) of the bigram grammar."""
    W = len(word_trans)
    B, init = np.asarray(B, dtype=np.float64), np.asarray(init, dtype=np.float64)
    assert n >= 2 and B.shape == (W, W) and init.shape == (W,)
    first = 1 + W * (n - 1)
    R = first + 2 * W
    entry = first + np.arange(W)
    row_of = np.empty((W, n), dtype=np.int64)
    row_of[:, 1:] = 1 + np.arange(W)[:, None] * (n - 1) + np.arange(n - 1)[None, :]
    row_of[:, 0] = first + W + np.arange(W)
    trans = np.full((R, R), np.inf)
    row_word = np.full(R, -1, dtype=np.int64)
    for w in range(W):
        rows = row_of[w]
        row_word[rows] = w
        trans[np.ix_(rows, rows)] = np.asarray(word_trans[w], dtype=np.float64)
        trans[rows[0], 0] = init[w]
        trans[rows[0], entry[w]] = 0.0
        trans[entry[w], row_of[:, n - 1]] = B[:, w]
    return trans, row_word < 0, row_word, [int(r) for r in row_of[:, n - 1]], entry, row_of


def _lse(x, axis=0):
    """max + log(sum exp(x - max)) along `axis`; -inf where the maximum is -inf (before any subtraction)."""
    x = np.asarray(x)
    m = x.max(axis=axis)
    none = np.isneginf(m)
    mm = np.where(none, 0, m).astype(x.dtype)
    with np.errstate(divide="ignore"):
        r = mm + np.log(np.exp(x - np.expand_dims(mm, axis)).sum(axis=axis))
    return np.where(none, -np.inf, r).astype(x.dtype)


def forward_backward(E, is_nes, trans, ends, dtype=np.float64):
    """(la, lb, gamma, logp) -- `O.forward_backward`, or for another dtype the same recursion, row by row, in that dtype."""
    if np.dtype(dtype) == np.float64:
        return O.forward_backward(np.asarray(E, dtype=np.float64), is_nes, trans, ends)
    E, trans = np.asarray(E, dtype=dtype), np.asarray(trans, dtype=dtype)
    R, T = E.shape
    NEG = dtype(-np.inf)
    preds = [np.flatnonzero(~np.isinf(trans[r])) for r in range(R)]
    succs = [np.flatnonzero(~np.isinf(trans[:, r])) for r in range(R)]
    la = np.full((R, T), NEG, dtype=dtype)
    for c in range(T):
        for r in range(R):
            if r == 0 and c == 0:
                la[0, 0] = -E[0, 0]
                continue
            terms = []
            for o in preds[r]:
                if is_nes[o] or is_nes[r]:
                    if o < r:
                        terms.append(la[o, c] - trans[r, o])
                elif c > 0:
                    terms.append(la[o, c - 1] - trans[r, o])
            if terms:
                la[r, c] = _lse(np.array(terms, dtype=dtype)) - E[r, c]
    lb = np.full((R, T), NEG, dtype=dtype)
    end_set = set(int(e) for e in ends)
    for c in range(T - 1, -1, -1):
        for r in range(R - 1, -1, -1):
            terms = []
            if c == T - 1 and r in end_set:
                terms.append(dtype(0.0))
            for s in succs[r]:
                if is_nes[s] or is_nes[r]:
                    if s > r:
                        terms.append(lb[s, c] - trans[s, r] - E[s, c])
                elif c + 1 < T:
                    terms.append(lb[s, c + 1] - trans[s, r] - E[s, c + 1])
            if terms:
                lb[r, c] = _lse(np.array(terms, dtype=dtype))
    logp = _lse(np.array([la[e, T - 1] for e in ends], dtype=dtype))
    with np.errstate(invalid="ignore"):
        gamma = np.exp(la + lb - logp)
    gamma[np.isnan(gamma)] = 0.0
    return la, lb, gamma, logp


def q_from_matrices(la, lb, logp, trans, row_word, entry, row_of):
    """post [T, W] by the formula; logp = -inf: every row is zero.  gamma is exp(la + lb - logp)."""
    W, n = row_of.shape
    T = la.shape[1]
    post = np.zeros((T, W), dtype=la.dtype)
    if np.isinf(logp):
        return post
    with np.errstate(invalid="ignore", over="ignore"):
        gamma = np.exp(la + lb - logp)
    gamma[np.isnan(gamma)] = 0.0
    last = row_of[:, n - 1]
    Bm = np.asarray(trans)[np.ix_(entry, last)].T.astype(la.dtype)        # Bm[w, u] = trans[L_u, last_w]
    row_word = np.asarray(row_word)
    for w in range(W):
        with np.errstate(invalid="ignore", over="ignore"):
            leave = np.exp(la[last[w]][None, :] - Bm[w][:, None] + lb[entry] - logp)   # [u, t]
        leave[np.isnan(leave)] = 0.0
        post[:, w] = gamma[row_word == w].sum(axis=0) - leave.sum(axis=0)
    return np.maximum(post, 0.0)


def word_posteriors_bigram(E, is_nes, row_word, trans, ends, entry, row_of, dtype=np.float64):
    """(post [T, W], logp): the formula on `forward_backward`."""
    la, lb, gamma, logp = forward_backward(E, is_nes, trans, ends, dtype)
    return q_from_matrices(la, lb, logp, trans, row_word, entry, row_of), logp


def sweep(word_trans, B, init, Es, dtype=np.float64, end_mask=None):
    """(post [T, W], logp, gamma_sum [T, W]) -- the recursion of `forward_backward` on the bigram grammar, one column at a
    time over [W, n] arrays: Es [T, W, n] emission costs, word_trans [W, n, n] (to, from), ends = the last states (or
    end_mask [W, n]).  gamma_sum is sum_s gamma_t(w, s), the uncorrected per-word occupancy."""
    wt = np.asarray(word_trans, dtype=dtype)
    B, init, Es = np.asarray(B, dtype=dtype), np.asarray(init, dtype=dtype), np.asarray(Es, dtype=dtype)
    T, W, n = Es.shape
    NEG = dtype(-np.inf)
    if end_mask is None:
        end_mask = np.zeros((W, n), dtype=bool)
        end_mask[:, n - 1] = True
    AL = np.empty((T, W, n), dtype=dtype)
    a = np.full((W, n), NEG, dtype=dtype)
    for t in range(T):
        inner = _lse(a[:, None, :] - wt, axis=2)                           # [w, to]: from the previous column
        new = inner - Es[t]
        EN = _lse(new[:, n - 1][:, None] - B, axis=0)                      # entry row of w: last states of THIS column
        start = -init if t == 0 else np.full(W, NEG, dtype=dtype)
        new[:, 0] = _lse(np.stack([inner[:, 0], EN, start]), axis=0) - Es[t, :, 0]
        AL[t] = a = new
    ends_alpha = np.where(end_mask, a, NEG).reshape(-1)
    logp = _lse(ends_alpha)
    post, gsum = np.zeros((T, W), dtype=dtype), np.zeros((T, W), dtype=dtype)
    if np.isinf(logp):
        return post, logp, gsum
    b = np.full((W, n), NEG, dtype=dtype)
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            nxt = np.full((W, n), NEG, dtype=dtype)
            endt = np.where(end_mask, dtype(0.0), NEG).astype(dtype)
        else:
            nxt = _lse((b - Es[t + 1])[:, :, None] - wt, axis=1)           # [w, from]: into the column behind
            endt = np.full((W, n), NEG, dtype=dtype)
        nb = _lse(np.stack([endt, nxt]), axis=0)
        BE = nb[:, 0] - Es[t, :, 0]                                        # beta of the entry rows
        LV = _lse(BE[None, :] - B, axis=1)                                 # what last_v sees through the entry rows
        nb[:, n - 1] = _lse(np.stack([endt[:, n - 1], nxt[:, n - 1], LV]), axis=0)
        b = nb
        with np.errstate(invalid="ignore"):
            g = np.exp(AL[t] + b - logp)
            leave = np.exp(AL[t][:, n - 1] + LV - logp)
        g[np.isnan(g)] = 0.0
        leave[np.isnan(leave)] = 0.0
        gsum[t] = g.sum(axis=1)
        post[t] = gsum[t] - leave
    return np.maximum(post, 0.0), logp, gsum
