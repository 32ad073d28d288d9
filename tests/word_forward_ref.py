# -*- coding: utf-8 -*-
"""Forward scores of stacked word chains on the host (test infrastructure, no GPU): the recursion of DESIGN.md 4.25 over
all chains at once, in numpy.

Notation of `O.forward_backward`: costs trans[to, from], neg-log emissions E[s, t].  Per chain, log domain, fp64:

    column 0:   a[0] = -E[0, 0], every other row -inf
    column t:   a[s] = LSE(a[s-2] - c2[s], a[s-1] - c1[s], a[s] - c0[s]) - E[s, t]      s descending, in place
    LSE(x..) = m + log(sum exp(x - m)), m = max, the sum in the order written; -inf where m is -inf
    soft = -a[n-1] of the last column (+inf: no path)

An arc that does not exist costs +inf: its term is -inf and adds exp(-inf) = 0 to the sum, which is what leaving the term
out (`O.forward_backward`) gives.  The softmax over the vocabulary is NOT restated here: `vocabulary_posteriors` of
`sr.recognition.batch` is the one statement, imported below for the tests' convenience."""
import numpy as np

from sr.recognition.batch import vocabulary_posteriors  # noqa: F401  (the host softmax: imported, not restated)


def word_trans(rng, n, skip=False):
    """A left-to-right word of n states, trans[to, from]; skip: arcs s -> s + 2 as well (some left out, never all)."""
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.05, 0.6) if i < n - 1 else rng.uniform(0.0, 0.3)
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.8, 2.5)
        if skip and i < n - 2 and (i == 0 or rng.random() < 0.6):
            t[i + 2, i] = rng.uniform(1.5, 4.0)
    return t


def chain_costs(trans_list):
    """(c0, c1, c2) [W, n]: the self, next and skip arc INTO state s of every word, +inf where there is none."""
    W, n = len(trans_list), len(trans_list[0])
    c0, c1, c2 = (np.full((W, n), np.inf) for _ in range(3))
    for w, t in enumerate(trans_list):
        t = np.asarray(t, dtype=np.float64)
        assert t.shape == (n, n)
        for s in range(n):
            c0[w, s] = t[s, s]
            if s >= 1:
                c1[w, s] = t[s, s - 1]
            if s >= 2:
                c2[w, s] = t[s, s - 2]
    return c0, c1, c2


def lse(terms):
    """Log-sum-exp over the first axis of terms [k, W], summed in the order of the rows."""
    terms = np.asarray(terms, dtype=np.float64)
    m = terms.max(axis=0)
    none = np.isneginf(m)
    ref = np.where(none, 0.0, m)
    s = np.zeros(terms.shape[1])
    for x in terms:
        s = s + np.exp(x - ref)
    with np.errstate(divide="ignore"):
        out = ref + np.log(s)
    out[none] = -np.inf
    return out


def forward_alpha(E, c0, c1, c2):
    """E [W, n, T] -> log-alphas [W, n, T] of every chain (T >= 1)."""
    W, n, T = E.shape
    al = np.full((W, n, T), -np.inf)
    a = np.full((W, n), -np.inf)
    a[:, 0] = -E[:, 0, 0]
    al[:, :, 0] = a
    for t in range(1, T):
        for s in range(n - 1, -1, -1):
            terms = []
            if s >= 2:
                terms.append(a[:, s - 2] - c2[:, s])
            if s >= 1:
                terms.append(a[:, s - 1] - c1[:, s])
            terms.append(a[:, s] - c0[:, s])
            a[:, s] = lse(terms) - E[:, s, t]
        al[:, :, t] = a
    return al


def soft_costs(E, c0, c1, c2):
    """E [W, n, T] -> soft [W] = -log P of every chain (its end row is its last); T = 0: +inf."""
    W, n, T = E.shape
    if T == 0:
        return np.full(W, np.inf)
    return -forward_alpha(E, c0, c1, c2)[:, n - 1, T - 1]


def soft_costs_batch(nll, offsets, trans_list):
    """The [U, W] matrix from a likelihood matrix nll [N, W n] (word w, state s in column w n + s) and frame offsets [U + 1]."""
    W, n = len(trans_list), len(trans_list[0])
    c = chain_costs(trans_list)
    nll = np.asarray(nll, dtype=np.float64)
    out = np.empty((len(offsets) - 1, W))
    for u in range(len(offsets) - 1):
        x = nll[offsets[u]:offsets[u + 1]]
        out[u] = soft_costs(x.T.reshape(W, n, len(x)), *c)
    return out
