# -*- coding: utf-8 -*-
"""The cell of the lane = chain Viterbi without back-pointers (viterbi_chain_lanes_kernel, gh_viterbi_chain.hip) is
    min(min(c2 + p2, c1 + p1), c0 + p0) + e,  then one more minimum against +inf,
in IEEE minNum (v_min_f64: a NaN operand loses), where the lane = row kernel tries the candidates in the order r-2, r-1, r
with a strict `<` from +inf and then maps NaN to +inf.  No GPU here: both formulations in numpy (np.fmin is minNum) over
EVERY combination of special and ordinary values, bit for bit -- the argument DESIGN 4.2 makes, executed.  The GPU
comparison of the two kernels is tests/test_gpu_chain_lanes.py."""
import itertools

import numpy as np

VALUES = [np.inf, -np.inf, np.nan, 0.0, 1.5, -2.25, 3.0, 1e308, -1e308]


def compare_form(v2, v1, v0, e):
    best = np.inf
    for v in (v2, v1, v0):
        if v < best:
            best = v
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.float64(best) + np.float64(e)
    return np.inf if c != c else c


def min_form(v2, v1, v0, e):
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.fmin(np.fmin(np.float64(v2), np.float64(v1)), np.float64(v0))
        return np.fmin(m + np.float64(e), np.inf)


def test_min_form_equals_compare_form_on_every_combination():
    n = 0
    for v2, v1, v0, e in itertools.product(VALUES, repeat=4):
        a = np.float64(compare_form(v2, v1, v0, e))
        b = np.float64(min_form(v2, v1, v0, e))
        assert a.tobytes() == b.tobytes(), (v2, v1, v0, e, a, b)
        n += 1
    assert n == len(VALUES) ** 4


def test_missing_candidates_are_plus_inf_candidates():
    """A row without the r-2 (or r-1) arc carries +inf as that arc's cost: c + p is +inf, or NaN against p = -inf, and
    neither changes the minimum -- leaving the candidate out (the first rows of a chain) is the same cell."""
    for p, v1, v0, e in itertools.product(VALUES, repeat=4):
        with np.errstate(invalid="ignore"):
            v2 = np.float64(np.inf) + np.float64(p)
        a = np.float64(min_form(v2, v1, v0, e))
        with np.errstate(invalid="ignore", over="ignore"):
            b = np.float64(np.fmin(np.fmin(np.float64(v1), np.float64(v0)) + np.float64(e), np.inf))
        assert a.tobytes() == b.tobytes(), (p, v1, v0, e, a, b)


def test_zeros_of_opposite_sign_are_the_only_difference():
    """minNum may order -0 below +0 where `<` does not: the two forms then agree in value, not necessarily in the sign bit."""
    for v2, v1, v0, e in itertools.product([0.0, -0.0, 1.0, np.inf, np.nan], repeat=4):
        a, b = compare_form(v2, v1, v0, e), min_form(v2, v1, v0, e)
        assert a == b or (a != a and b != b), (v2, v1, v0, e, a, b)
