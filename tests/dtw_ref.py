# -*- coding: utf-8 -*-
"""Column-vectorised restatement of `oracle.ref_numpy.dtw` (the reference's dtw, decode.py:7-77) and the seeded inputs of
tests/test_gpu_dtw.py.

`oracle.ref_numpy.dtw` is a triple Python loop (n * n * T interpreted steps); `dtw_ref` takes one numpy step per column
over the [n, n] candidate matrix and is checked against the oracle, costs and paths, in tests/test_dtw_ref_host.py.  It
differs from the oracle in three documented places:
  * a walk that would leave column 0 in a row other than 0 raises ValueError (the oracle wraps to column -1 there and may
    never return);
  * `stable=True` ranks a beamed column with a stable argsort -- ascending (value, row), the order gh_dtw.hip documents --
    where the oracle's default argsort is free to order equal values either way;
  * a genuine cost of exactly -1.0 is not taken for a beam mark (the oracle keeps its marks in the cost matrix itself).

The builders at the end make the inputs of the GPU tests from fixed seeds; the host test file asserts for every one of
them that no decision of the DP is closer than `min_gap` > 1e-9, that the walk ends and that the input reaches the branch
it is named for."""
from math import isinf

import numpy as np

LD = np.longdouble


def _rel_gap(a, b):
    """(b - a) / max(|a|, |b|) for finite a <= b; +inf when either is not finite."""
    if not (np.isfinite(a) and np.isfinite(b)):
        return np.inf
    m = max(abs(a), abs(b))
    return 0.0 if m == 0.0 and a == b else (b - a) / max(m, np.finfo(np.float64).tiny)


def _cell_gaps(cand):
    """Smallest relative gap between winner and runner-up over the rows of `cand` [r, k] whose winner is finite."""
    if cand.shape[1] < 2 or cand.shape[0] == 0:
        return np.inf
    two = np.partition(cand, 1, axis=1)[:, :2]                # NaN sorts last: a row with a NaN has no finite winner below
    has_nan = np.isnan(cand).any(axis=1)
    ok = ~has_nan & np.isfinite(two[:, 0]) & np.isfinite(two[:, 1])
    if not ok.any():
        return np.inf
    w, r = two[ok, 0], two[ok, 1]
    m = np.maximum(np.maximum(np.abs(w), np.abs(r)), np.finfo(np.float64).tiny)
    return float(np.min((r - w) / m))


def dtw_ref(E, trans, beam=np.inf, stable=True, want_stats=False):
    """-> (costs [n, T], path [K, 2], min_gap[, stats]) of `oracle.ref_numpy.dtw(E, trans, beam)`.

    Every origin of the previous column is a candidate, +inf arcs included; np.argmin per row: the first NaN wins, else
    the first minimum; min(inf, nan) keeps inf.  A cell ranked >= beam in its finished column (and not infinite) is
    marked: row 0 of the next column drops it from its candidate list (its index is mapped back through the surviving
    origins), the rows >= 1 read it as +inf; it is returned as -1 in the last column and +inf elsewhere.
    min_gap: over all cells with a finite winner the smallest relative gap between the winning candidate and the
    runner-up, and over beamed columns the smallest gap between the cells ranked beam - 1 and beam.
    stats (want_stats): counts of the branches a case is meant to reach."""
    E = np.asarray(E, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    n, T = E.shape
    assert T > 1 and n > 1 and trans.shape == (n, n)          # decode.py:22
    pruning = not isinf(beam)
    if pruning:
        beam = int(beam)
        assert beam >= 0
    costs = np.full((n, T), np.inf)
    bp = np.zeros((n, T), dtype=np.int64)
    prev = np.full(n, np.inf)                                 # column -1 is the (still untouched) last column
    marked = np.zeros(n, dtype=bool)
    min_gap = np.inf
    stats = dict(nan_cells=0, all_inf_cells=0, neginf_cells=0, marks=0, last_marks=0, last_marks_hi=0, cut_ties=0, cut_ties_cross=0)
    with np.errstate(invalid="ignore"):
        for j in range(T):
            eff = np.where(marked, np.inf, prev)
            cand = trans + eff[None, :]
            k = np.argmin(cand, axis=1)
            best = cand[np.arange(n), k]
            min_gap = min(min_gap, _cell_gaps(cand[1:]))
            surv = np.flatnonzero(~marked)
            if surv.size == 0:
                raise ValueError("attempt to get argmin of an empty sequence")
            cand0 = trans[0, surv] + prev[surv]
            k0 = int(np.argmin(cand0))
            k[0], best[0] = surv[k0], cand0[k0]
            min_gap = min(min_gap, _cell_gaps(cand0[None, :]))
            c = best + E[:, j]
            nan_c = np.isnan(best)
            c = np.where(c < np.inf, c, np.inf)
            if j == 0:
                c[0], k[0] = E[0, 0], 0
                nan_c[0] = False
            stats["nan_cells"] += int(nan_c.sum())
            stats["all_inf_cells"] += int(np.all(np.isposinf(cand), axis=1)[1:].sum())
            stats["neginf_cells"] += int(np.isneginf(c).sum())
            bp[:, j] = k
            marked = np.zeros(n, dtype=bool)
            if pruning:
                order = np.argsort(c, kind="stable") if stable else np.argsort(c)
                for i in order[beam:]:
                    if not isinf(c[i]):
                        marked[i] = True
                if 0 < beam < n:
                    s = np.sort(c)
                    g = _rel_gap(s[beam - 1], s[beam])
                    min_gap = min(min_gap, g)
                    stats["cut_ties"] += int(g == 0.0)
                    if g == 0.0:                              # equal finite costs on both sides of the cut, in two waves?
                        rows = np.flatnonzero(c == s[beam])
                        stats["cut_ties_cross"] += int(rows.min() < 64 <= rows.max())
                stats["marks"] += int(marked.sum())
                if j == T - 1:
                    stats["last_marks"] = int(marked.sum())
                    stats["last_marks_hi"] = int(marked[64:].sum())
            costs[:, j] = np.where(marked, -1.0 if j == T - 1 else np.inf, c)
            prev = c
    i, j = n - 1, T - 1
    path = []
    while i != 0 or j != 0:
        if j == 0:
            raise ValueError("back-trace left the matrix: cell (0,0) is not reachable from the end cell")
        i, j = int(bp[i, j]), j - 1
        path.append([i, j])
    path = np.array(path, dtype=np.int64).reshape(-1, 2)
    if want_stats:
        return costs, path, float(min_gap), stats
    return costs, path, float(min_gap)


def distance_matrix_ld(x, y, kind="euclid", var=None):
    """E[i, j] = dist(x[j], y[i]) in np.longdouble, rounded to fp64 once at the end.  kind: "euclid" (||x - y||) or
    "mahalanobis" (0.5 log((2 pi)^D prod var) + 0.5 sum (x - y)^2 / var, hmm_state.py:48-58).  Where the reference's
    fp64 (2 pi)^D prod var overflows (D > 386 or so) the distance IS +inf -- that overflow belongs to the operation."""
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    diff = x[None, :, :] - y[:, None, :]                      # [n, T, D]
    if kind == "euclid":
        return np.sqrt(np.sum(diff * diff, axis=2)).astype(np.float64)
    assert kind == "mahalanobis"
    D = x.shape[1]
    v64 = np.asarray(var, dtype=np.float64)
    v = v64.astype(LD)
    two_pi = LD(8) * np.arctan(LD(1))
    logdet = LD(0.5) * (LD(D) * np.log(two_pi) + np.sum(np.log(v), axis=1))
    out = (logdet[:, None] + LD(0.5) * np.sum(diff * diff / v[:, None, :], axis=2)).astype(np.float64)
    with np.errstate(over="ignore"):
        overflow = np.isinf(np.float64(2.0 * np.pi) ** D * np.prod(v64, axis=1))
    out[overflow] = np.inf
    return out


def row_sequence(path, n, T):
    """The template row of every frame from a dtw path (rows of columns 0 .. T-2; frame T-1 sits on row n-1)."""
    rows = np.empty(T, dtype=np.int64)
    rows[T - 1] = n - 1
    assert len(path) == T - 1
    rows[path[:, 1]] = path[:, 0]
    return rows


# ------------------------------------------------------------------------------------------- seeded inputs (GPU tests)
def ltr_trans(rng, n, skip=2):
    """Left-to-right arc costs: self loop, and arcs up to +skip rows; trans[i, o] = cost of going from row o to row i."""
    trans = np.full((n, n), np.inf)
    for o in range(n):
        trans[o, o] = rng.uniform(0.1, 0.5)
        for s in range(1, skip + 1):
            if o + s < n:
                trans[o + s, o] = rng.uniform(0.3, 1.0) + 0.4 * (s - 1) * rng.uniform(0.5, 1.0)
    return trans


def frames_along(rng, y, T, noise=0.3):
    """T frames that run through the template rows from first to last."""
    n = len(y)
    return y[np.minimum(np.arange(T) * n // T, n - 1)] + noise * rng.normal(size=(T, y.shape[1]))


def skip_for(n, T):
    """Arcs long enough for T columns to reach row n - 1 from row 0 (and at least +2)."""
    return max(2, -(-(n - 1) // max(T - 1, 1)) + 1)


def make_case(seed, n, D, lengths, skip=None):
    """Templates, variances in [0.5, 2] (every logdet is positive), arcs and utterances from one seed."""
    rng = np.random.default_rng(seed)
    if skip is None:
        skip = 8 if n >= 128 else 2
    y = rng.normal(size=(n, D)) * 2.0
    var = rng.uniform(0.5, 2.0, size=(n, D))
    trans = ltr_trans(rng, n, skip)
    xs = [frames_along(rng, y, T) for T in lengths]
    return dict(n=n, D=D, y=y, var=var, trans=trans, xs=xs, seed=seed)


def case_dists(case, kind, u=None):
    """High-precision distance matrices of a case's utterances ("dist": the euclid matrices, handed to the device)."""
    var = case["var"] if kind == "mahalanobis" else None
    k = "mahalanobis" if kind == "mahalanobis" else "euclid"
    us = range(len(case["xs"])) if u is None else [u]
    return [distance_matrix_ld(case["xs"][i], case["y"], k, var) for i in us]


def nan_trans(rng, n):
    """The pattern of G5's `trans_skip` scaled to n rows.  An empty segment e has a NaN self loop and a -inf arc to e + 1:
    row e always finds a NaN candidate (cost +inf), and so does row e + 1 (-inf + inf) -- these -inf arcs lie OFF the
    winning path, which passes the pair through a +3 skip arc.  The arc from row n - 2 to the last row is -inf as well:
    that one lies ON the winning path (end cost -inf once row n - 2 is reached, a NaN candidate before)."""
    trans = ltr_trans(rng, n, 3 if n < 128 else 8)
    for e in sorted({n // 3} | ({n // 2} if n >= 16 else set())):
        trans[e, e] = np.nan
        trans[e + 1, e] = -np.inf
    trans[n - 1, n - 2] = -np.inf
    return trans


def nan_case(seed, n, D):
    """Three utterances under `nan_trans`: one that ends in the column in which the last row first reads the -inf arc from
    a finite origin (end cost -inf; a column later the +inf arcs out of that -inf cell have turned every other row into
    NaN candidates), a longer one and one too short to reach the end."""
    trans = nan_trans(np.random.default_rng(seed + 7), n)
    with np.errstate(invalid="ignore"):
        probe = dtw_ref(np.ones((n, 4 * n)), trans)[0]
    t_end = int(np.flatnonzero(np.isneginf(probe[n - 1]))[0]) + 1
    case = make_case(seed, n, D, (t_end + 12, t_end, max(3, t_end // 3)), skip=3 if n < 128 else 8)
    case["trans"] = trans
    return case


FIT_W, FIT_PER_WORD = 3, 4


def fit_case(n, D):
    """gh_fit_dtw: FIT_W words with their own templates and arcs, FIT_PER_WORD utterances per word, interleaved in the
    batch (utterance u belongs to word u % FIT_W); lengths from 2 frames up."""
    rng = np.random.default_rng(4000 + 10 * n + D)
    y = rng.normal(size=(FIT_W, n, D)) * 2.0
    trans = np.array([ltr_trans(rng, n, 2) for _ in range(FIT_W)])
    U = FIT_W * FIT_PER_WORD
    lengths = [2, n + 3, 2 * n + 1] + [int(t) for t in rng.integers(max(2, n // 2), 2 * n + 9, size=U - 3)]
    utt_word = np.arange(U, dtype=np.int32) % FIT_W
    xs = [frames_along(rng, y[utt_word[u]], lengths[u]) for u in range(U)]
    return dict(n=n, D=D, y=y, trans=trans, xs=xs, utt_word=utt_word)


def fit_reference(case):
    """[(costs, path, min_gap) per utterance] against the utterance's own word."""
    out = []
    for u, x in enumerate(case["xs"]):
        w = case["utt_word"][u]
        out.append(dtw_ref(distance_matrix_ld(x, case["y"][w], "euclid"), case["trans"][w]))
    return out


def int_tie_case(n, T, beam):
    """Integer distance matrix and arcs (all sums exact) in which equal finite costs sit on both sides of the beam cut, in
    different waves when n > 64: every row may be entered from row 0 at the same integer price."""
    rng = np.random.default_rng(1000 + n)
    trans = np.full((n, n), np.inf)
    for o in range(n):
        trans[o, o] = 1.0
        if o + 1 < n:
            trans[o + 1, o] = 2.0
    trans[1:, 0] = 3.0                                         # row 0 fans out to every row: equal costs across the waves
    E = rng.integers(1, 3, size=(n, T)).astype(np.float64)
    E[0, :] = 1.0
    return E, trans, beam


# ----------------------------------------------------------------------------------- the launch rule, restated (host)
def launch_form(n, D, kind):
    """(back-pointer type, staged, waves) gh_launch_dtw picks: staged when the arcs (and, for the built-in distances, the
    template rows and variances) fit 96 KB of LDS and D <= 4 threads."""
    threads = (n + 63) & ~63
    extra = n * n * 8 + (0 if kind == "dist" else n * D * 8 * (2 if kind == "mahalanobis" else 1))
    return ("u8" if n <= 255 else "u16", extra <= 96 * 1024 and D <= 4 * threads, threads // 64)


def window_len(n):
    """Back-pointer columns the back-trace stages into LDS at a time."""
    threads = (n + 63) & ~63
    return 18 * threads // (1 if n <= 255 else 2) // n


# ------------------------------------------------------------------------------------------------ the cases, by name
BATCH_LENGTHS = (2, 90, 3, 17, 64, 5, 33, 2, 71, 45, 10)
KINDS2 = ("euclid", "mahalanobis")
KINDS3 = ("euclid", "mahalanobis", "dist")
INST = ((2, 13, 9), (5, 13, 14), (64, 13, 70), (65, 5, 70), (100, 5, 60), (128, 5, 40), (255, 5, 45), (256, 5, 45),
        (300, 5, 47), (5, 257, 14))
STRIDE_D = {5: (1, 39, 63, 64, 65, 128, 129, 255, 256), 70: (127, 128, 129, 512)}
BEAM_N = (5, 64, 65, 130)
NAN_N = (5, 70, 256)
WINDOW_N = (2, 5, 64, 300)


def _job(name, case, kinds, beams=(np.inf,), needs=()):
    return dict(name=name, case=case, kinds=tuple(kinds), beams=tuple(beams), needs=tuple(needs))


def _build_jobs():
    jobs = []
    for n, D, T in INST:
        jobs.append(_job("inst-n%d-D%d" % (n, D), make_case(11 * n + D + (1 if n == 256 else 0), n, D, (T, T + 5)), KINDS3))
    for n, Ds in STRIDE_D.items():
        for D in Ds:
            jobs.append(_job("stride-n%d-D%d" % (n, D), make_case(7 * n + D, n, D, (12 if n == 5 else 40,)), KINDS2))
    for n in BEAM_N:
        T = {5: 20, 64: 70, 65: 70, 130: 40}[n]
        case = make_case(300 + n, n, 5, (T,))
        # a second utterance that stalls one row short of the end: the last row is finite but not the cheapest cell of
        # the last column, so a narrow beam marks it there (-1 in the highest row, in the second wave for n > 64)
        case["xs"].append(frames_along(np.random.default_rng(350 + n), case["y"][:n - 1], T))
        jobs.append(_job("beam-n%d" % n, case, KINDS2, (1, 2, n - 1, n, n + 5),
                         ("last_marks",) + (("last_marks_hi",) if n > 64 else ())))
    for n in NAN_N:
        jobs.append(_job("nan-n%d" % n, nan_case(500 + n, n, 5), KINDS2, (np.inf,),
                         ("nan_cells", "neginf_cells", "all_inf_cells")))
    for n in WINDOW_N:
        w = window_len(n)
        for T in (w - 1, w, w + 1, 2 * w + 1):
            jobs.append(_job("window-n%d-T%d" % (n, T), make_case(700 + n + T, n, 5, (T, 2), skip=skip_for(n, w - 1)),
                             ("euclid",)))
    for n in (5, 70):
        jobs.append(_job("batch-n%d" % n, make_case(900 + n, n, 5, BATCH_LENGTHS), KINDS2, (np.inf, 3 if n == 5 else 20)))
    return jobs


_JOBS = None
_REFS = {}


def jobs():
    global _JOBS
    if _JOBS is None:
        _JOBS = {j["name"]: j for j in _build_jobs()}
    return _JOBS


def job_names(prefix):
    return [k for k in jobs() if k.startswith(prefix + "-")]


def reference(name, kind, beam):
    """[(costs, path, min_gap, stats) per utterance] of a named case: dtw_ref on the long-double distance matrices.
    Computed once and shared; callers must not write into it."""
    key = (name, "euclid" if kind == "dist" else kind, beam)
    if key not in _REFS:
        job = jobs()[name]
        out = []
        for E in case_dists(job["case"], key[1]):
            r = dtw_ref(E, job["case"]["trans"], beam=beam, want_stats=True)
            for a in r[:2]:
                a.setflags(write=False)
            out.append(r)
        _REFS[key] = out
    return _REFS[key]


def row0_drop_case():
    """Integer case for "row 0 drops a marked origin": under beam 1 row 0 is marked in column 1, so cell (0, 2) finds only
    +inf candidates and points at the first SURVIVING origin (row 1), not at origin 0; the end cell is out of reach and
    points at row 0, so the walk (4,3) -> (0,2) -> (1,1) -> (0,0) passes through that cell."""
    n, T = 5, 4
    trans = np.full((n, n), np.inf)
    for o in range(n):
        trans[o, o] = 1.0
        if o + 1 < n:
            trans[o + 1, o] = 2.0
    E = np.ones((n, T))
    E[0, 1:] = 5.0
    return E, trans, 1
