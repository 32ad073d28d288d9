# -*- coding: utf-8 -*-
"""Word posteriors of the word-loop grammar on the host (test infrastructure, no GPU).

Notation of `O.loop_grammar` / `O.forward_backward`: log alpha la, log beta lb, log P, costs trans[to, from]; the loop row
is Lr = 1 + W (n - 1), last_w the last state of word w.  Every path visits one or more emitting cells per column -- more
than one exactly where it hops through the loop row -- and a path's WORD AT FRAME t is the word of the LAST emitting cell
it visits in column t (the boundary frame belongs to the entering word, the rule of the begin times).

    q_t(w) = sum_s gamma_t(w, s)  -  exp( la[last_w, t] - trans[Lr, last_w] + lb[Lr, t] - logP )

`word_posteriors` is that formula on `O.forward_backward`; `brute_force` enumerates every path with its word at every
frame; `confidence` is the mean of q over a decoded word's frames."""
import numpy as np

from oracle import ref_numpy as O


def word_posteriors(E, is_nes, row_word, trans, ends, W, n):
    """(post [T, W], logp) from O.forward_backward.  logp = -inf: every row is zero."""
    R, T = E.shape
    la, lb, gamma, logp = O.forward_backward(E, is_nes, trans, ends)
    post = np.zeros((T, W))
    if np.isinf(logp):
        return post, logp
    Lr = 1 + W * (n - 1)
    row_word = np.asarray(row_word)
    for w in range(W):
        rows = np.flatnonzero(row_word == w)
        last = 1 + w * (n - 1) + (n - 2)                                  # state n - 1 of word w
        assert row_word[last] == w
        with np.errstate(invalid="ignore", over="ignore"):
            leave = np.exp(la[last] - trans[Lr, last] + lb[Lr] - logp)
        leave[np.isnan(leave)] = 0.0
        post[:, w] = gamma[rows].sum(axis=0) - leave
    return np.maximum(post, 0.0), logp


def brute_force(E, is_nes, row_word, trans, ends, W):
    """(post [T, W], logp) by enumeration of every path from (row 0, column 0) to an end row in the last column, under
    the same-column rule of A6 / A13 (an arc that touches a non-emitting row stays in its column and runs to a higher
    row).  The word of a path at frame t is the word of the last emitting cell it visits in column t."""
    R, T = E.shape
    succs = [np.flatnonzero(~np.isinf(trans[:, r])) for r in range(R)]
    end_set = set(int(e) for e in ends)
    weight = np.zeros((T, W))
    total = [0.0]

    def walk(r, c, cost, words):
        # words: word of the last emitting cell of every finished column, plus the running one of column c
        if c == T - 1 and r in end_set:
            p = np.exp(-cost)
            total[0] += p
            for t, w in enumerate(words):
                weight[t, w] += p
        for s in succs[r]:
            s = int(s)
            same = is_nes[s] or is_nes[r]
            if same:
                if s <= r:
                    continue
                c2 = c
            else:
                c2 = c + 1
                if c2 >= T:
                    continue
            w2 = words
            if not is_nes[s]:
                w2 = (words[:c2] + (int(row_word[s]),)) if len(words) > c2 else words + (int(row_word[s]),)
            walk(s, c2, cost + trans[s, r] + E[s, c2], w2)

    walk(0, 0, E[0, 0], ())
    if total[0] == 0.0:
        return np.zeros((T, W)), -np.inf
    return weight / total[0], np.log(total[0])


def confidence(post, labels, begins, T):
    """Mean of post[t, label_k] over begin_k <= t < end_k, end_k = begin_{k+1}, the last word ends at T.  No words: an
    empty array."""
    labels = [int(l) for l in labels]
    begins = [int(b) for b in begins]
    ends = begins[1:] + [int(T)]
    return np.array([post[b:e, l].sum() / (e - b) for l, b, e in zip(labels, begins, ends)], dtype=np.float64)
