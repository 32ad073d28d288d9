# -*- coding: utf-8 -*-
"""TEST INFRASTRUCTURE: the wide online session restated AT BIT LEVEL in numpy -- what csrc/gh_viterbi_online_wide.hip
writes and what csrc/gh_online_wide_settle.hip reads.

`WideSweep` is the column step of viterbi_online_wide_kernel over 64 word lanes: the same candidates in the same order,
strict '<', one 32-bit decision word per column and lane with gh_loop_hb(N, SKIP) bits at the bottom -- the in-word bits
from the top (state N - 1 first; with skip arcs b_a = "s - 1 beats s - 2" then b_b = "self beats both" for s >= 2), then
`cand == rm`, b_l, b_s -- kept in a ring of `ring_cols` columns, column j at j % ring_cols.

`WideSettle` is online_wide_settle_kernel followed by the commit mode of online_wide_segment_kernel: a mask of live states
per lane, the two 64-bit ballots of the loop-row hop as Python integers, the lowest set lane of the `eq` ballot, the set
size from "one lane has a mask and none has two bits", and the label rule of the segment walk.  It reads nothing but the
ring and the carried column.  tests/test_online_wide_settle_host.py holds it against `online_settle_ref.SettledDecode`
on `online_ref.CarriedDecode`, which work on graph rows and know nothing of lanes, masks or bits."""
import numpy as np

LANES = 64


def loop_hb(n, skip):
    return n + 2 + (n - 2 if skip else 0)


def ballot(b):
    """The 64-bit ballot of a boolean per lane, as an int."""
    return sum(1 << int(l) for l in np.flatnonzero(np.asarray(b, dtype=bool)))


class WideSweep:
    def __init__(self, trans, W, n, ring_cols=None):
        """trans [R, R]: the dense arc costs of an `O.loop_grammar` graph of W words x n states."""
        trans = np.asarray(trans, dtype=np.float64)
        self.W, self.n = W, n
        self.Lr = Lr = 1 + W * (n - 1)
        self.row = np.array([[Lr + 1 + w if s == 0 else 1 + w * (n - 1) + (s - 1) for w in range(W)] for s in range(n)])
        self.c0, self.c1, self.c2 = (np.full((n, LANES), np.inf) for _ in range(3))
        self.cin, self.cin0, self.cout = (np.full(LANES, np.inf) for _ in range(3))
        for w in range(W):
            for s in range(n):
                self.c0[s, w] = trans[self.row[s, w], self.row[s, w]]
                if s >= 1:
                    self.c1[s, w] = trans[self.row[s, w], self.row[s - 1, w]]
                if s >= 2:
                    self.c2[s, w] = trans[self.row[s, w], self.row[s - 2, w]]
            self.cin[w], self.cin0[w], self.cout[w] = trans[self.row[0, w], Lr], trans[self.row[0, w], 0], trans[Lr, self.row[n - 1, w]]
        self.skip = bool(np.isfinite(self.c2).any())
        self.hb = loop_hb(n, self.skip)
        self.ring_cols = ring_cols
        self.reset()

    def reset(self):
        self.t = 0
        self.prev = np.full((self.n, LANES), np.inf)
        self.ring = {}                                # ring position -> uint32 [64]

    def word_of(self, j):
        return self.ring[j if self.ring_cols is None else j % self.ring_cols]

    def push(self, E):
        """E [R, t]: the emission costs of the chunk's frames on the graph's rows."""
        n, W = self.n, self.W
        for k in range(E.shape[1]):
            e = np.zeros((n, LANES))
            e[:, :W] = E[self.row, k]
            prev = self.prev if self.t > 0 else np.full((n, LANES), np.inf)
            new = np.empty((n, LANES))
            word = np.zeros(LANES, dtype=np.uint64)
            base0 = self.c0[0] + prev[0]
            for s in range(n - 1, 0, -1):
                v0, v1 = self.c0[s] + prev[s], self.c1[s] + prev[s - 1]
                if self.skip and s >= 2:
                    v2 = self.c2[s] + prev[s - 2]
                    m = np.minimum(v1, v2)
                    word = (word << np.uint64(1)) | (v1 < v2).astype(np.uint64)
                    word = (word << np.uint64(1)) | (v0 < m).astype(np.uint64)
                    best = np.minimum(v0, m)
                else:
                    word = (word << np.uint64(1)) | (v0 < v1).astype(np.uint64)
                    best = np.minimum(v0, v1)
                new[s] = best + e[s]
            cand = new[n - 1] + self.cout
            rm = cand.min()
            word = (word << np.uint64(1)) | (cand == rm).astype(np.uint64)
            cs = (0.0 if self.t == 0 else np.inf) + self.cin0
            cl = rm + self.cin
            m2 = np.minimum(cl, cs)
            word = (word << np.uint64(1)) | (cl < cs).astype(np.uint64)
            word = (word << np.uint64(1)) | (base0 < m2).astype(np.uint64)
            new[0] = np.minimum(base0, m2) + e[0]
            assert int(word.max()) < 1 << self.hb <= 1 << 32
            self.ring[self.t if self.ring_cols is None else self.t % self.ring_cols] = word.astype(np.uint32)
            self.prev = new
            self.t += 1


class WideSettle:
    def __init__(self, sweep):
        self.sw = sweep
        self.reset()

    def reset(self):
        self.anchor = None                            # (column, word, state)
        self.words = []
        self.flag = 0
        self.passed = []                              # (column, hop ballot, eq ballot) of every hop the walks took

    @property
    def settled_frames(self):
        return 0 if self.anchor is None else self.anchor[0] + 1

    def row_of(self, word, state):
        return int(self.sw.row[state, word])

    def _codes(self, hb):
        """In-word origin of every state s >= 1 of a lane from its decision bits: s - code."""
        n, HB = self.sw.n, self.sw.hb
        codes, before = {}, 0
        for s in range(n - 1, 0, -1):
            if self.sw.skip and s >= 2:
                b_a, b_b = (hb >> (HB - 1 - before)) & 1, (hb >> (HB - 2 - before)) & 1
                codes[s] = 0 if b_b else (1 if b_a else 2)
                before += 2
            else:
                codes[s] = 0 if (hb >> (HB - 1 - before)) & 1 else 1
                before += 1
        return codes

    def settle(self):
        """online_wide_settle_kernel: the candidate anchor (column, word, state), or the old one."""
        sw = self.sw
        n, W, T = sw.n, sw.W, sw.t
        lo = 0 if self.anchor is None else self.anchor[0]
        mask = [0] * LANES
        if T >= 2:
            for w in range(W):
                mask[w] = sum(int(sw.prev[s, w] < np.inf) << s for s in range(n))
        j = T - 1
        active = any(mask) and j > lo
        while active:
            col = [int(v) & ((1 << sw.hb) - 1) for v in sw.word_of(j)]
            hops = ballot([(mask[l] & 1) and not (col[l] & 1) and (col[l] >> 1) & 1 for l in range(LANES)])
            eq = ballot([l < W and (col[l] >> 2) & 1 for l in range(LANES)])
            for l in range(LANES):
                if (mask[l] & 1) and not (col[l] & 1):
                    mask[l] &= ~1
                    if not (col[l] >> 1) & 1:
                        self.flag |= 2
            if hops:
                self.passed.append((j, hops, eq))
                if not eq:
                    self.flag |= 2
                else:
                    mask[(eq & -eq).bit_length() - 1] |= 1 << (n - 1)      # __ffsll(eq) - 1
            for l in range(LANES):
                if mask[l]:
                    codes, nm = self._codes(col[l]), mask[l] & 1
                    for s in range(1, n):
                        if (mask[l] >> s) & 1:
                            nm |= 1 << (s - codes[s])
                    mask[l] = nm
            j -= 1
            some = ballot([m != 0 for m in mask])
            many = ballot([bin(m).count("1") > 1 for m in mask])
            if some and not some & (some - 1) and not many:
                w = some.bit_length() - 1
                return (j, w, (mask[w] & -mask[w]).bit_length() - 1)
            if not some or j <= lo:
                if self.anchor is not None:
                    self.flag |= 2
                active = False
        return self.anchor

    def segment(self, new):
        """The commit mode of online_wide_segment_kernel: the words between the old anchor and `new`, oldest first."""
        sw = self.sw
        n, W = sw.n, sw.W
        stop = self.anchor
        lo = 0 if stop is None else stop[0]
        j, bw, bs = new
        out, pending, kind = [], bw, 0                # pending: the label of the run the walk is in (-1: a non-emitting row)
        while j > lo:
            if kind == 0:
                hb = int(sw.word_of(j)[bw]) & ((1 << sw.hb) - 1)
                if bs >= 1:
                    bs -= self._codes(hb)[bs]
                    j -= 1
                elif hb & 1:
                    j -= 1
                elif (hb >> 1) & 1:
                    kind = 1
                    if pending >= 0:
                        out.append(pending)
                    pending = -1
                else:
                    self.flag |= 2
                    break
            else:
                eq = ballot([l < W and (int(sw.word_of(j)[l]) >> 2) & 1 for l in range(LANES)])
                if not eq:
                    self.flag |= 2
                    break
                bw, bs, kind = (eq & -eq).bit_length() - 1, n - 1, 0
                pending = bw
        if stop is not None:
            if (bw, bs) != (stop[1], stop[2]):
                self.flag |= 2
        elif pending >= 0:
            out.append(pending)                       # no anchor: the walk ended in column 0, the first word counts
        return out[::-1]

    def commit(self):
        """Advances the anchor; returns the words settled by THIS call."""
        new = self.settle()
        if new is None or new == self.anchor:
            return []
        words = self.segment(new)
        self.anchor = new
        self.words = self.words + words
        return words
