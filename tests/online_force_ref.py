# -*- coding: utf-8 -*-
"""TEST INFRASTRUCTURE: the FORCED COMMIT of an online decode, restated on `online_ref.CarriedDecode` and
`online_settle_ref.SettledDecode` -- what gh_online_force computes (csrc/gh_online_force.hip), followed by the ordinary
commit.

For a stream with T frames, old anchor column lo (-1: none) and bound M, let c* = T - 1 - M.  Nothing happens if T < 2,
c* < 0, c* <= lo, or the chosen end of the newest column (`CarriedDecode.result`'s rule: the last of equal minima over the
end rows) is +inf.  Otherwise:
  1. BACK WALK: A is the cell in which the trace of the chosen end ARRIVES in column c* (`SettledDecode.arrive`, repeated);
  2. FORWARD MARKING: from {A} in column c*, column by column up to T - 1, the emitting cells whose trace arrives in a marked
     cell of the column below;
  3. PRUNE: every emitting cell of the newest column that is finite and not marked gets +inf in `cd.col`.
Nothing else is written; `sd.commit()` called next finds an anchor in a column >= c*.

A dead cell (+inf) has back-pointers too -- the reference's arg-min over +inf costs -- and they may end in a row without
predecessor; such a trace arrives nowhere and is never marked.  A finite cell has finite predecessors only, so what step 3
prunes does not depend on how dead cells are marked on the way."""
import numpy as np

from oracle import ref_numpy as O


def chosen_end(cd):
    """(index of the chosen end or -1, its cost) of the newest column: `CarriedDecode.result`'s rule."""
    if cd.t == 0:
        return -1, np.inf
    best, bi = np.inf, -1
    for k, e in enumerate(cd.end_rows):
        if best >= cd.col[e]:
            best, bi = cd.col[e], k
    return bi, best


def arrive(cd, r, j):
    """The row of column j - 1 in which the trace of the cell (r, j) arrives, or None where the trace ends before."""
    i, c = int(r), int(j)
    while c == j:
        i, c = (int(v) for v in cd.bp[c][i])
        if i == O._NOPTR:
            return None
    assert c == j - 1
    return i


def marked_cells(cd, c_star, A):
    """The emitting rows of the newest column whose trace arrives in the cell (A, c_star): step 2."""
    marked = {int(A)}
    emitting = [r for r in range(cd.R) if not cd.is_nes[r]]
    for j in range(c_star + 1, cd.t):
        marked = {r for r in emitting if arrive(cd, r, j) in marked}
    return marked


def force(cd, sd, max_tail):
    """Steps 1 - 3 on the carried column of `cd`; `sd` gives the old anchor.  Returns dict(pruned: cells set to +inf,
    cell: (c*, A) or None where nothing had to be done, marked: the marked rows of the newest column)."""
    assert max_tail >= 1
    T = cd.t
    lo = -1 if sd.anchor is None else sd.anchor[0]
    c_star = T - 1 - int(max_tail)
    nothing = dict(pruned=0, cell=None, marked=None)
    if T < 2 or c_star < 0 or c_star <= lo:
        return nothing
    bi, cost = chosen_end(cd)
    if bi < 0 or not np.isfinite(cost):
        return nothing
    r = cd.end_rows[bi]
    for j in range(T - 1, c_star, -1):
        r = arrive(cd, r, j)
        assert r is not None, "the trace of a finite cell reached a row without predecessor"
    marked = marked_cells(cd, c_star, r)
    assert cd.end_rows[bi] in marked
    pruned = 0
    for q in range(cd.R):
        if not cd.is_nes[q] and np.isfinite(cd.col[q]) and q not in marked:
            cd.col[q] = np.inf
            pruned += 1
    return dict(pruned=pruned, cell=(c_star, r), marked=marked)


def forced_commit(cd, sd, max_tail):
    """What `OnlineDecoder.commit` does for one stream with `max_tail` set: the natural commit; where more than max_tail
    frames stay unsettled, force and commit again.  Returns (the words settled by this call, cells pruned)."""
    new = sd.commit()
    pruned = 0
    if cd.t - sd.settled_frames > max_tail:
        pruned = force(cd, sd, max_tail)["pruned"]
        new = new + sd.commit()
    return new, pruned
