# -*- coding: utf-8 -*-
"""TEST INFRASTRUCTURE: the wide BIGRAM online session restated AT BIT LEVEL in numpy -- what
csrc/gh_viterbi_bigram_online_wide.hip writes and what csrc/gh_online_bigram_wide_settle.hip reads.

`BigramWideSweep` is the column step of viterbi_bigram_online_wide_kernel over 64 word lanes: the same candidates in the
same order, strict '<', one 32-bit record per column and lane with gh_bigram_wide_hb(N, SKIP) bits at the bottom -- the
in-word bits from the top (state N - 1 first; with skip arcs b_a = "s - 1 beats s - 2" then b_b = "self beats both" for
s >= 2), then 6 bits of predecessor word v (the first minimum of last[v] + B[v][w]; 0 where every candidate is +inf), b_l,
b_s -- kept in a ring of `ring_cols` columns, column j at j % ring_cols.

`BigramWideSettle` is online_bigram_wide_settle_kernel followed by the commit mode of online_bigram_wide_segment_kernel: a
mask of live states per lane; THE HOP -- a lane with b0 && !b_s && b_l names v in its own record, lane w gets bit N - 1 iff
some hopper names v == w, before the in-word decisions of the same column are applied; the set size from "one lane has a
mask and none has two bits"; the label rule of the segment walk, an entry row left through the 6-bit field of the same
record (with the arc-mask fallback of the kernel).  It reads nothing but the ring and the carried column.

`HopLog` is `online_settle_ref.SettledDecode` -- which walks graph rows and back-pointers and knows nothing of lanes, masks
or bits -- that notes every hop its walks take: per column the (word, predecessor word) pairs of the live first states that
were entered through their entry row.  The input conditions of the tests are read from it.
tests/test_online_bigram_wide_settle_host.py holds the bit level against the row level."""
import numpy as np

from online_settle_ref import SettledDecode

LANES = 64


def bigram_wide_hb(n, skip):
    return n + 7 + (n - 2 if skip else 0)


def ballot(b):
    """The 64-bit ballot of a boolean per lane, as an int."""
    return sum(1 << int(l) for l in np.flatnonzero(np.asarray(b, dtype=bool)))


class HopLog(SettledDecode):
    """SettledDecode on a bigram graph of W words x n states that logs the hops of its walks: hops[column] is the set of
    (word, predecessor word) of the live first states whose trace leaves through their entry row in that column."""

    def __init__(self, cd, row_word, W, n, cols=None):
        """cols: the list the caller appends every carried column to (what `cd.push` returns); with it `tied` counts the
        hops whose entry row had equal minimal candidates (the lowest word wins: np.argmin's first minimum)."""
        self.W, self.n, self.Lr = W, n, 1 + W * (n - 1)
        self.hops, self.cols, self.tied = {}, cols, set()
        super().__init__(cd, row_word)

    def arrive(self, r, j):
        first = self.Lr + self.W
        if first <= r < first + self.W:
            i, c = (int(v) for v in self.cd.bp[j][r])
            if c == j and self.Lr <= i < first:
                o = int(self.cd.bp[j][i][0])
                self.hops.setdefault(j, set()).add((r - first, (o - 1) // (self.n - 1)))
                if self.cols is not None:
                    cand = self.cd.trans[i, self.cd.preds[i]] + self.cols[j][self.cd.preds[i]]
                    if np.isfinite(cand.min()) and np.sum(cand == cand.min()) > 1:
                        assert self.cd.preds[i][int(np.argmin(cand))] == o
                        self.tied.add((j, r - first))
        return super().arrive(r, j)

    def two_word_columns(self):
        """Columns in which live first states hop to at least two different words."""
        return sum(len({v for _, v in h}) >= 2 for h in self.hops.values())

    def crossing_hops(self):
        """Hops from a word of one 16-lane group to a word of another."""
        return sum(w // 16 != v // 16 for h in self.hops.values() for w, v in h)


class BigramWideSweep:
    def __init__(self, trans, W, n, ring_cols=None):
        """trans [R, R]: the dense arc costs of a `packed_bigram_lattice` graph of W words x n states."""
        trans = np.asarray(trans, dtype=np.float64)
        self.W, self.n = W, n
        self.Lr = Lr = 1 + W * (n - 1)
        self.row = np.array([[Lr + W + w if s == 0 else 1 + w * (n - 1) + (s - 1) for w in range(W)] for s in range(n)])
        self.c0, self.c1, self.c2 = (np.full((n, LANES), np.inf) for _ in range(3))
        self.cin0 = np.full(LANES, np.inf)
        self.bg = np.full((LANES, LANES), np.inf)       # bg[v][w]: last state of word v -> entry row of word w
        for w in range(W):
            for s in range(n):
                self.c0[s, w] = trans[self.row[s, w], self.row[s, w]]
                if s >= 1:
                    self.c1[s, w] = trans[self.row[s, w], self.row[s - 1, w]]
                if s >= 2:
                    self.c2[s, w] = trans[self.row[s, w], self.row[s - 2, w]]
            self.cin0[w] = trans[self.row[0, w], 0]
            assert trans[self.row[0, w], Lr + w] == 0.0                     # (the arc entry row -> state 0 costs 0)
            self.bg[:W, w] = trans[Lr + w, self.row[n - 1]]
        self.bg_in = [ballot(np.isfinite(self.bg[:, w])) for w in range(LANES)]
        self.skip = bool(np.isfinite(self.c2).any())
        self.hb = bigram_wide_hb(n, self.skip)
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
        one = np.uint64(1)
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
                    word = (word << one) | (v1 < v2).astype(np.uint64)
                    word = (word << one) | (v0 < m).astype(np.uint64)
                    best = np.minimum(v0, m)
                else:
                    word = (word << one) | (v0 < v1).astype(np.uint64)
                    best = np.minimum(v0, v1)
                new[s] = best + e[s]
            # entry[w] = min_v (last[v] + B[v][w]), the first minimum; every candidate +inf: v = 0
            cand = new[n - 1][:, None] + self.bg
            arg = np.argmin(cand, axis=0)
            entry = cand[arg, np.arange(LANES)]
            word = (word << np.uint64(6)) | arg.astype(np.uint64)
            cs = (0.0 if self.t == 0 else np.inf) + self.cin0
            m2 = np.minimum(entry, cs)
            word = (word << one) | (entry < cs).astype(np.uint64)
            word = (word << one) | (base0 < m2).astype(np.uint64)
            new[0] = np.minimum(base0, m2) + e[0]
            assert int(word.max()) < 1 << self.hb <= 1 << 32
            self.ring[self.t if self.ring_cols is None else self.t % self.ring_cols] = word.astype(np.uint32)
            self.prev = new
            self.t += 1


class BigramWideSettle:
    def __init__(self, sweep):
        self.sw = sweep
        self.reset()

    def reset(self):
        self.anchor = None                            # (column, word, state)
        self.words = []
        self.flag = 0
        self.passed = []                              # (column, [(hopper lane, named word)]) of every hop the settle walks took
        self.entries = 0                              # entry rows the segment walks passed

    @property
    def settled_frames(self):
        return 0 if self.anchor is None else self.anchor[0] + 1

    def row_of(self, word, state):
        return int(self.sw.row[state, word])

    def _codes(self, hb):
        """In-word origin of every state s >= 1 of a lane from its record: s - code."""
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
        """online_bigram_wide_settle_kernel: the candidate anchor (column, word, state), or the old one."""
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
            hit = [0] * LANES                           # the hit table: every lane's own slot zeroed, hoppers store at [v]
            hoppers = []
            for l in range(LANES):
                if (mask[l] & 1) and not (col[l] & 1):
                    mask[l] &= ~1
                    v = (col[l] >> 2) & 63
                    if not (col[l] >> 1) & 1 or v >= W:
                        self.flag |= 2
                    else:
                        hit[v] = 1
                        hoppers.append((l, v))
            if hoppers:
                self.passed.append((j, hoppers))
            for l in range(LANES):
                if hit[l]:
                    mask[l] |= 1 << (n - 1)
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
        """The commit mode of online_bigram_wide_segment_kernel: the words between the old anchor and `new`, oldest first."""
        sw = self.sw
        n, W = sw.n, sw.W
        stop = self.anchor
        lo = 0 if stop is None else stop[0]
        j, bw, bs = new
        out, pending, kind = [], bw, 0                # pending: the label of the run the walk is in (-1: a non-emitting row)
        while j > lo:
            hb = int(sw.word_of(j)[bw]) & ((1 << sw.hb) - 1)
            if kind == 1:                             # the entry row of word bw: the predecessor its record names
                v, arcs = (hb >> 2) & 63, sw.bg_in[bw]
                if not (arcs >> v) & 1:
                    v = (arcs & -arcs).bit_length() - 1 if arcs else -1
                if v < 0 or v >= W:
                    self.flag |= 2
                    break
                bw, bs, kind = v, n - 1, 0
                pending = bw
            elif bs >= 1:
                bs -= self._codes(hb)[bs]
                j -= 1
            elif hb & 1:
                j -= 1
            elif (hb >> 1) & 1:
                kind = 1
                self.entries += 1
                if pending >= 0:
                    out.append(pending)
                pending = -1
            else:
                self.flag |= 2
                break
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
