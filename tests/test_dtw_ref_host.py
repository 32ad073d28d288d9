# -*- coding: utf-8 -*-
"""tests/dtw_ref.py on the CPU: the column-vectorised `dtw_ref` against the oracle's triple loop, its stable beam order,
its ValueError for an unreachable origin -- and the inputs of tests/test_gpu_dtw.py: every seeded case keeps all of its
decisions further apart than 1e-9 (so a path can be compared exactly on the device), lets the oracle's walk end, and
reaches the branch it is named for."""
import numpy as np
import pytest

import dtw_ref as R
from conftest import load_golden
from oracle import ref_numpy as O

GAP = 1e-9


def same_as_oracle(E, trans, beam):
    with np.errstate(invalid="ignore"):
        oc, op = O.dtw(E, trans, beam=beam)
    c, p, gap = R.dtw_ref(E, trans, beam=beam)
    assert gap > 0                                            # no ties: the oracle's default argsort has no freedom
    np.testing.assert_array_equal(c, oc)
    np.testing.assert_array_equal(p, np.asarray(op).reshape(-1, 2))


def test_matches_oracle_on_G5():
    g = load_golden("G5_dtw")
    x, y, var, trans = g["x"], g["y"], g["var"], g["trans"]
    Ee, Em = O.distance_matrix(x, y, "euclid"), O.distance_matrix(x, y, "mahalanobis", var)
    for tag, E, tr, beam in (("euclid", Ee, trans, np.inf), ("mahal", Em, trans, np.inf), ("beam3", Em, trans, 3),
                             ("beam2", Ee, trans, 2), ("skip", Em, g["trans_skip"], np.inf)):
        same_as_oracle(E, tr, beam)
        c, p, _ = R.dtw_ref(E, tr, beam=beam)
        np.testing.assert_array_equal(p, g["path_" + tag])    # (and the recorded reference run itself)
        np.testing.assert_array_equal(np.isinf(c), np.isinf(g["costs_" + tag]))


@pytest.mark.parametrize("n", [2, 3, 5, 17])
def test_matches_oracle_on_random_graphs(n):
    rng = np.random.default_rng(n)
    for T in sorted({T for T in (2, n - 1, n, 3 * n) if T >= 2}):
        trans = R.ltr_trans(rng, n, 2)
        E = rng.uniform(0.5, 3.0, size=(n, T))
        for beam in (np.inf, 1, 2, n - 1, n, n + 3):
            if beam >= 1:
                same_as_oracle(E, trans, beam)


@pytest.mark.parametrize("n", [5, 17])
def test_matches_oracle_with_nan_and_neginf_arcs(n):
    rng = np.random.default_rng(40 + n)
    trans = R.nan_trans(rng, n)
    seen = dict(nan_cells=0, neginf_cells=0)
    for T in (3, 4, n, 3 * n):
        E = rng.uniform(0.5, 3.0, size=(n, T))
        same_as_oracle(E, trans, np.inf)
        st = R.dtw_ref(E, trans, want_stats=True)[3]
        for k in seen:
            seen[k] += st[k]
    assert seen["nan_cells"] > 0 and seen["neginf_cells"] > 0


def brute_force_stable(E, trans, beam):
    """The oracle's loop with the beamed column ranked by sorted (value, row) pairs."""
    n, T = E.shape
    costs = np.full((n, T), np.inf)
    marks = np.zeros((n, T), dtype=bool)
    for j in range(T):
        for i in range(n):
            if i == 0 and j == 0:
                costs[0, 0] = E[0, 0]
                continue
            cand = [trans[i, o] + (np.inf if (j == 0 or marks[o, j - 1]) else costs[o, j - 1]) for o in range(n)
                    if not (i == 0 and j > 0 and marks[o, j - 1])]
            costs[i, j] = min(np.inf, min(cand) + E[i, j])
        order = [i for _, i in sorted((costs[i, j], i) for i in range(n))]
        for i in order[beam:]:
            marks[i, j] = np.isfinite(costs[i, j])
    return costs, marks


@pytest.mark.parametrize("n,beam", [(5, 3), (70, 40)])
def test_stable_beam_marks_the_larger_rows_among_equal_costs(n, beam):
    E, trans, beam = R.int_tie_case(n, 8, beam)
    c, p, gap, st = R.dtw_ref(E, trans, beam=beam, stable=True, want_stats=True)
    assert gap == 0.0 and st["cut_ties"] > 0                  # equal finite costs on both sides of the cut
    if n > 64:
        assert st["cut_ties_cross"] > 0                       # ... in rows of different waves
    bc, bm = brute_force_stable(E, trans, beam)
    marked = (np.isinf(c) & np.isfinite(bc)) | (c == -1.0)
    np.testing.assert_array_equal(marked, bm)
    np.testing.assert_array_equal(c[~marked], bc[~marked])
    assert not (bc == -1.0).any()
    for j in range(E.shape[1]):                                # among equal finite costs the larger rows are the marked ones
        for v in np.unique(bc[np.isfinite(bc[:, j]), j]):
            rows = np.flatnonzero(bc[:, j] == v)
            m = bm[rows, j]
            assert not (m[:-1] & ~m[1:]).any()


def test_row0_drop_case_walks_through_the_dropped_origin():
    E, trans, beam = R.row0_drop_case()
    same_as_oracle(E, trans, beam)
    np.testing.assert_array_equal(R.dtw_ref(E, trans, beam=beam)[1], [[0, 2], [1, 1], [0, 0]])


def test_unreachable_origin_raises():
    trans = np.array([[0.3, np.inf], [0.7, -np.inf]])          # (the oracle does not return from this one)
    with pytest.raises(ValueError, match="back-trace left the matrix"):
        R.dtw_ref(np.ones((2, 4)), trans)


# ------------------------------------------------------------------------------------ the inputs of test_gpu_dtw.py
FORMS = {(2, 13): ("u8", True, 1), (5, 13): ("u8", True, 1), (64, 13): ("u8", True, 1),          # staged uint8, one wave
         (65, 5): ("u8", True, 2), (100, 5): ("u8", True, 2),                                    # staged uint8, multi-wave
         (128, 5): ("u8", False, 2), (255, 5): ("u8", False, 4),                                 # unstaged uint8 by size
         (256, 5): ("u16", False, 4), (300, 5): ("u16", False, 5),                               # unstaged uint16
         (5, 257): ("u8", False, 1)}                                                             # unstaged by D > 4 threads


def test_instantiation_cases_take_their_launch_form():
    assert sorted(FORMS) == sorted((n, D) for n, D, _ in R.INST)
    for (n, D), form in FORMS.items():
        for kind in R.KINDS3:
            assert R.launch_form(n, D, kind) == form, (n, D, kind)
    # no n reaches the staged 16-bit form: 256 rows need 512 KB for the arcs alone
    assert not any(R.launch_form(n, 1, "dist")[1] for n in range(256, 1025))
    for D in R.STRIDE_D[5]:                                    # one wave: the frame is staged with strides q = 0 .. 3
        assert all(R.launch_form(5, D, k)[1] for k in R.KINDS2)
    # two waves: rows, variances and arcs of 70 templates at D >= 127 exceed 96 KB -- these run unstaged; a staged launch
    # of more than one wave with D > its thread count (a stride q >= 1 of 128 or more) does not exist at any n
    for D in R.STRIDE_D[70]:
        assert not any(R.launch_form(70, D, k)[1] for k in R.KINDS2)
    assert not any(R.launch_form(n, ((n + 63) & ~63) + 1, "euclid")[1] for n in range(65, 1025))


def test_window_cases_straddle_the_window():
    assert [R.window_len(n) for n in R.WINDOW_N] == [576, 230, 18, 9]
    for n in R.WINDOW_N:
        w = R.window_len(n)
        Ts = sorted(len(R.jobs()[k]["case"]["xs"][0]) for k in R.job_names("window") if k.startswith("window-n%d-" % n))
        assert Ts == [w - 1, w, w + 1, 2 * w + 1]
        for k in R.job_names("window"):
            if k.startswith("window-n%d-" % n):
                rc, rp = R.reference(k, "euclid", np.inf)[0][:2]
                assert np.isfinite(rc[-1, -1]) and len(set(rp[:, 0])) > 1     # a walk that changes rows


@pytest.mark.parametrize("name", list(R.jobs()))
def test_gpu_input_is_decisive_and_reaches_its_branch(name):
    job = R.jobs()[name]
    n = job["case"]["n"]
    seen = {}
    for kind in job["kinds"]:
        for beam in job["beams"]:
            for costs, path, gap, st in R.reference(name, kind, beam):    # (dtw_ref returned: the walk ends)
                assert gap > GAP, (name, kind, beam, gap)
                for k, v in st.items():
                    seen[k] = seen.get(k, 0) + v
                assert not (costs == -1.0).any() or st["last_marks"] > 0     # no genuine cost of -1: that value is the mark
    for k in job["needs"]:
        assert seen[k] > 0, (name, k)
    if name.startswith("nan-"):
        ends = [r[0][-1, -1] for r in R.reference(name, "euclid", np.inf)]
        assert any(np.isneginf(e) for e in ends) and any(np.isposinf(e) for e in ends)
    if name.startswith("batch-"):
        assert sorted(len(x) for x in job["case"]["xs"]) == sorted(R.BATCH_LENGTHS) and len(R.BATCH_LENGTHS) == 11
        assert min(R.BATCH_LENGTHS) == 2 and max(R.BATCH_LENGTHS) == 90
        assert sum(st["marks"] for beam in job["beams"] if beam < n for _, _, _, st in R.reference(name, "euclid", beam)) > 0


@pytest.mark.parametrize("n,D", [(2, 5), (5, 5), (32, 5), (2, 64), (5, 64), (32, 64)])
def test_fit_input_is_decisive(n, D):
    case = R.fit_case(n, D)
    assert sorted(np.bincount(case["utt_word"])) == [R.FIT_PER_WORD] * R.FIT_W
    assert list(case["utt_word"][:R.FIT_W]) == list(range(R.FIT_W))                 # interleaved
    for costs, path, gap in R.fit_reference(case):
        assert gap > GAP
