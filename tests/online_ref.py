# -*- coding: utf-8 -*-
"""TEST INFRASTRUCTURE: the CARRIED form of the oracle's decode (`oracle.ref_numpy.decode_fill` / `decode_states`, i.e.
decode_hmm_states, decode.py:80-146) -- what online decoding computes.

The reference fills its cost matrix column by column, and a column reads the previous column (arcs between emitting rows)
and itself (arcs touching a non-emitting row, rows already visited) only.  `CarriedDecode` therefore keeps ONE column and
the back-pointers of all columns, takes the emissions of a chunk of any length (0 frames included) and can at any time
select the end and trace back as the reference does behind its last column.

Contract (tests/test_online_host.py, on `O.loop_grammar` graphs): every carried column is bitwise the whole decode's
column, and the result after k frames is bitwise `O.decode_states` of the first k frames -- end costs, chosen end, path.
The one place where the reference's sweep is not causal is its column wrap at c == 0 (`costs[o, c - 1]` reads the LAST
column, decode.py:109-114): with more than one frame that column is still +inf, with exactly one frame it is the column
being filled, in which -- in a loop grammar, whose first states come last in row order -- every row such an arc can read
is still +inf as well.  The carried form reads +inf there; the k = 1 case of the tests pins that this changes nothing.
"""
import numpy as np

from oracle import ref_numpy as O


class CarriedDecode:
    def __init__(self, is_nes, trans, end_rows):
        self.is_nes = np.asarray(is_nes, dtype=bool)
        self.trans = np.asarray(trans, dtype=np.float64)
        self.end_rows = [int(e) for e in end_rows]
        self.R = len(self.is_nes)
        self.preds = [np.flatnonzero(~np.isinf(self.trans[r])) for r in range(self.R)]
        self.reset()

    def reset(self):
        self.t = 0                                    # frames taken = absolute column of the next frame
        self.col = np.full(self.R, np.inf)            # the previous column
        self.bp = []                                  # back-pointers [R, 2] of every column taken

    def push(self, E):
        """E [R, t]: emission costs of the chunk's frames (0 on non-emitting rows), t >= 0.  Returns the columns [R, t]."""
        E = np.asarray(E, dtype=np.float64).reshape(self.R, -1)
        out = np.empty(E.shape)
        for k in range(E.shape[1]):
            c = self.t
            prev = self.col if c > 0 else np.full(self.R, np.inf)      # (c == 0: see the module docstring)
            col = np.full(self.R, np.inf)
            bp = np.full((self.R, 2), O._NOPTR, dtype=np.int64)
            for r in range(self.R):
                if r == 0 and c == 0:
                    col[0] = E[0, k]
                    continue
                if len(self.preds[r]) == 0:
                    continue
                best_v = None
                best_pt = None
                for o in self.preds[r]:
                    same = self.is_nes[o] or self.is_nes[r]
                    v = self.trans[r, o] + (col[o] if same else prev[o])
                    if best_v is None or v < best_v:
                        best_v, best_pt = v, (int(o), c if same else c - 1)
                if best_pt == (r, c):
                    raise NameError("FUCKED")  # decode.py:120-121
                bp[r] = best_pt
                col[r] = min(col[r], best_v + E[r, k])
            self.col = col
            self.bp.append(bp)
            self.t += 1
            out[:, k] = col
        return out

    def result(self):
        """(end costs [n_end], index of the chosen end or -1, path [K, 2] end -> start) for the frames taken so far."""
        if self.t == 0:
            return np.full(len(self.end_rows), np.inf), -1, np.zeros((0, 2), dtype=np.int64)
        ec = self.col[self.end_rows]
        best, bi = np.inf, -1
        for k, v in enumerate(ec):
            if best >= v:                             # the last of equal end points (decode.py:129-134)
                best, bi = v, k
        i, j = self.end_rows[bi], self.t - 1
        path = []
        while j != 0:
            i, j = self.bp[j][i]
            path.append([i, j])
            if len(path) > self.R * self.t:
                raise RuntimeError("back-trace does not terminate")
        return ec.copy(), bi, np.array(path, dtype=np.int64).reshape(-1, 2)
