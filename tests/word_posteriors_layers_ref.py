# -*- coding: utf-8 -*-
"""Word posteriors of the K-layer lattice on the host (test infrastructure, no GPU, no `sr` package).

Rows as `O.build_state_sequences(n, word_trans, [[0 .. W-1]] * K)` lays them out: row 0 = NES_0, then per layer k the
P = W n emitting rows (word w, state s at k (P + 1) + 1 + w n + s) and the non-emitting row NES_{k+1} = (k + 1)(P + 1).
Notation of `O.forward_backward`: log alpha la, log beta lb, log P, costs trans[to, from]; last_{k,w} the last state of word w
in layer k.  A path's WORD AT FRAME t is the word of the LAST emitting cell it visits in column t:

    q_t(k, w) = sum_s gamma_t(k, w, s)  -  exp( la[last_{k,w}, t] - trans[NES_{k+1}, last_{k,w}] + lb[NES_{k+1}, t] - logP )
    q_t(w)    = sum over k of q_t(k, w)

(the subtracted term: leaving word w of layer k through NES_{k+1} in column t; 0 for the last layer, lb[NES_K] = -inf).

  `layers_graph`            (row_word, row_state, is_nes, trans, ends) of the lattice
  `emissions`               E [R, T] from per-state costs [T, W n]
  `q_from_matrices`         the formula on given la, lb, log P: (q [T, W], qk [T, K, W])
  `word_posteriors_layers`  the formula on `forward_backward` (float64: the oracle itself; np.longdouble: the same recursion
                            in that dtype): THE restatement
  `sweep`                   the same recursion written per column over [K, W, n] arrays with the layer sum in the device
                            kernel's order: the restatement at sizes where a row-by-row recursion in Python takes long.  The
                            host tests hold it to `word_posteriors_layers` at 1e-12.
`brute_force` and `confidence` come from tests/word_posteriors_ref.py: they take any graph with is_nes and row_word."""
import numpy as np

from oracle import ref_numpy as O
from word_posteriors_ref import brute_force, confidence  # noqa: F401  (re-exported)
from word_posteriors_bigram_ref import _lse, forward_backward


def layers_graph(word_trans, n, K):
    return O.build_state_sequences(n, [np.asarray(t, dtype=np.float64) for t in word_trans], [list(range(len(word_trans)))] * K)


def emissions(costs, row_word, row_state, n):
    """E [R, T]: row r scores column row_word[r] n + row_state[r] of costs [T, W n]; non-emitting rows cost 0."""
    row_word, row_state = np.asarray(row_word), np.asarray(row_state)
    nes = row_word < 0
    col = np.where(nes, 0, row_word * n + row_state)
    costs = np.asarray(costs)
    return np.where(nes[:, None], costs.dtype.type(0.0), costs[:, col].T)


def q_from_matrices(la, lb, logp, trans, W, n, K):
    """(q [T, W], qk [T, K, W]) by the formula; logp = -inf: zeros.  A q(k, w) below 0 by rounding counts as 0; the layers
    are added in ascending order."""
    T = la.shape[1]
    qk = np.zeros((T, K, W), dtype=la.dtype)
    if np.isinf(logp):
        return qk.sum(axis=1), qk
    P = W * n
    trans = np.asarray(trans)
    for k in range(K):
        nxt = (k + 1) * (P + 1)
        for w in range(W):
            r0 = k * (P + 1) + 1 + w * n
            last = r0 + n - 1
            with np.errstate(invalid="ignore", over="ignore"):
                g = np.exp(la[r0:r0 + n] + lb[r0:r0 + n] - logp)
                leave = np.exp(la[last] - la.dtype.type(trans[nxt, last]) + lb[nxt] - logp)
            g[np.isnan(g)] = 0.0
            leave[np.isnan(leave)] = 0.0
            qk[:, k, w] = g.sum(axis=0) - leave
    qk = np.maximum(qk, 0.0)
    q = np.zeros((T, W), dtype=la.dtype)
    for k in range(K):
        q = q + qk[:, k]
    return q, qk


def word_posteriors_layers(E, is_nes, trans, ends, W, n, K, dtype=np.float64):
    """(q [T, W], logp, qk [T, K, W]): the formula on `forward_backward`."""
    la, lb, gamma, logp = forward_backward(E, is_nes, trans, ends, dtype)
    q, qk = q_from_matrices(la, lb, logp, trans, W, n, K)
    return q, logp, qk


def _layer_sum(qk):
    """sum over the layers (axis 0 of [K, W]) in the kernel's order: ((0 + 4) + (1 + 5)) + ((2 + 6) + (3 + 7)), absent
    layers add 0.0."""
    K = qk.shape[0]
    zero = np.zeros_like(qk[0])
    lane = [(qk[r] if r < K else zero) + (qk[r + 4] if r + 4 < K else zero) for r in range(4)]
    return (lane[0] + lane[1]) + (lane[2] + lane[3])


def sweep(word_trans, Es, K, dtype=np.float64, cin=None, cout=None):
    """(post [T, W], logp, gamma_sum [T, W]) -- the recursion of `forward_backward` on the K-layer lattice, one column at a
    time over [K, W, n] arrays, the way the device kernel runs it: Es [T, W, n] emission costs, word_trans [W, n, n]
    (to, from), entry / exit costs cin / cout [W] (default 0, as `layers_graph` builds them), ends = the last states of the
    last layer.  gamma_sum is sum_k sum_s gamma_t(k, w, s), the uncorrected per-word occupancy."""
    wt = np.asarray(word_trans, dtype=dtype)
    Es = np.asarray(Es, dtype=dtype)
    T, W, n = Es.shape
    assert K <= 8
    cin = np.zeros(W, dtype=dtype) if cin is None else np.asarray(cin, dtype=dtype)
    cout = np.zeros(W, dtype=dtype) if cout is None else np.asarray(cout, dtype=dtype)
    NEG = dtype(-np.inf)
    AL = np.empty((T, K, W, n), dtype=dtype)
    a = np.full((K, W, n), NEG, dtype=dtype)
    for t in range(T):
        inner = _lse(a[:, :, None, :] - wt[None], axis=3)                  # [k, w, to]: from the previous column
        new = inner - Es[t][None]
        nes = _lse(new[:, :, n - 1] - cout[None], axis=1)                  # NES_{k+1}: last states of THIS column
        nes_in = np.concatenate([[dtype(0.0) if t == 0 else NEG], nes[:-1]]).astype(dtype)
        new[:, :, 0] = _lse(np.stack([nes_in[:, None] - cin[None], inner[:, :, 0]]), axis=0) - Es[t, :, 0][None]
        AL[t] = a = new
    logp = _lse(a[K - 1, :, n - 1])
    post, gsum = np.zeros((T, W), dtype=dtype), np.zeros((T, W), dtype=dtype)
    if np.isinf(logp):
        return post, logp, gsum
    b = np.full((K, W, n), NEG, dtype=dtype)
    for t in range(T - 1, -1, -1):
        endt = np.full((K, W, n), NEG, dtype=dtype)
        if t == T - 1:
            nxt = np.full((K, W, n), NEG, dtype=dtype)
            endt[K - 1, :, n - 1] = 0.0
        else:
            nxt = _lse((b - Es[t + 1][None])[:, :, :, None] - wt[None], axis=2)   # [k, w, from]: into the column behind
        nb = _lse(np.stack([endt, nxt]), axis=0)
        bnes = _lse(nb[:, :, 0] - cin[None] - Es[t, :, 0][None], axis=1)   # beta of NES_k
        down = np.concatenate([bnes[1:], [NEG]]).astype(dtype)             # ... handed to layer k - 1; BNES_K = -inf
        lv = down[:, None] - cout[None]
        nb[:, :, n - 1] = _lse(np.stack([endt[:, :, n - 1], nxt[:, :, n - 1], lv]), axis=0)
        b = nb
        with np.errstate(invalid="ignore"):
            g = np.exp(AL[t] + b - logp)
            leave = np.exp(AL[t][:, :, n - 1] - cout[None] + down[:, None] - logp)
        g[np.isnan(g)] = 0.0
        leave[np.isnan(leave)] = 0.0
        gk = g.sum(axis=2)
        gsum[t] = _layer_sum(gk)
        post[t] = _layer_sum(np.maximum(gk - leave, 0.0))
    return post, logp, gsum
