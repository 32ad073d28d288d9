# -*- coding: utf-8 -*-
"""TEST INFRASTRUCTURE: the SETTLED PREFIX of an online decode, restated on `online_ref.CarriedDecode` -- what
gh_online_commit computes (csrc/gh_online_settle.hip).

From every emitting row of the newest column whose carried cost is finite, follow `cd.bp` until the column changes: that
is the cell in which the row's trace ARRIVES in the column below (a first state entered through the loop row passes the
loop row and the last state that fed it, both in its own column, on the way).  Repeat on the set of cells; it can only
shrink.  The first column, from T - 2 down, in which the set has one member holds the ANCHOR; the walk also ends in the
previous anchor, which every trace passes.  The settled words are `O.path_to_words` of the path from the anchor (included)
to the start."""
import numpy as np

from oracle import ref_numpy as O


class SettledDecode:
    def __init__(self, cd, row_word):
        self.cd, self.row_word = cd, np.asarray(row_word)
        self.reset()

    def reset(self):
        self.anchor = None                            # (column, row)
        self.words = []                               # the labels up to the anchor
        self.live = set()                             # the cells of the last walk's last column
        self._arrive = {}                             # (row, column) -> row: the back-pointers of a column never change

    @property
    def settled_frames(self):
        return 0 if self.anchor is None else self.anchor[0] + 1

    def arrive(self, r, j):
        """The cell of column j - 1 that the trace of the cell (r, j) arrives in."""
        if (r, j) not in self._arrive:
            i, c = r, j
            while c == j:
                i, c = (int(v) for v in self.cd.bp[c][i])
            assert c == j - 1
            self._arrive[r, j] = i
        return self._arrive[r, j]

    def path_from(self, r, j):
        """[row, column] cells from (r, j), included, back to the first cell visited in column 0."""
        path = [[r, j]]
        while j != 0:
            r, j = (int(v) for v in self.cd.bp[j][r])
            path.append([r, j])
        return np.array(path, dtype=np.int64)

    def commit(self):
        """Advances the anchor; returns the words settled by THIS call."""
        cd = self.cd
        live = {r for r in range(cd.R) if not cd.is_nes[r] and np.isfinite(cd.col[r])} if cd.t >= 2 else set()
        lo = 0 if self.anchor is None else self.anchor[0]
        j = cd.t - 1
        while live and j > lo:
            live = {self.arrive(r, j) for r in live}
            j -= 1
            if len(live) == 1:
                break
        self.live = live
        if len(live) != 1:
            assert self.anchor is None or not live    # the traces of live cells meet in the old anchor at the latest
            return []
        anchor = (j, next(iter(live)))
        assert self.anchor is None or anchor >= self.anchor
        if anchor == self.anchor:
            return []
        words = O.path_to_words(self.path_from(anchor[1], anchor[0]), cd.is_nes, self.row_word)
        assert words[:len(self.words)] == self.words
        new, self.anchor, self.words = words[len(self.words):], anchor, words
        return new
