# -*- coding: utf-8 -*-
"""tests/mfcc_ref.py pinned before it judges a kernel (CPU only): the extended-precision restatement of `mfcc_features`
against the reference project's own output (G15) and against the fp64 oracle on every geometry of the GPU sweep, at the
rtol = atol = 1e-9 the MFCC kernel is held to -- the measured deviation is printed and lies many orders below.  And what
the GPU tests (test_gpu_mfcc_geometry.py) rely on about their INPUTS: frame and step in samples, frame counts, which rows
and columns of the reference are exactly log10(eps)."""
import numpy as np
import pytest

import mfcc_ref as M
from conftest import load_golden
from oracle import ref_numpy as O

TOL = 1e-9


def deviation(got, want):
    """max |got - want| / (1 + |want|): below TOL / 2 implies assert_allclose(rtol = atol = TOL)."""
    return float(np.max(np.abs(got - want) / (1 + np.abs(want)))) if got.size else 0.0


def assert_close(got, want, what):
    assert got.shape == want.shape, what
    dev = deviation(got, want)
    assert np.allclose(got, want, rtol=TOL, atol=TOL), "%s: deviation %.3g" % (what, dev)
    return dev


def test_precision_of_the_reference_arithmetic():
    # a narrower long double computes the same text in fp64: nothing is skipped, the tolerances below still hold
    assert np.finfo(np.longdouble).eps <= np.finfo(np.float64).eps
    assert abs(float(M.PI) - np.pi) <= 4e-16
    assert M.LOG_EPS == np.log10(np.finfo(float).eps) and -15.66 < M.LOG_EPS < -15.65
    np.testing.assert_allclose(M.hamming(400).astype(float), np.hamming(400), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(M.hamming(1).astype(float), np.hamming(1))
    np.testing.assert_allclose(M.hamming(2).astype(float), np.hamming(2), rtol=0, atol=1e-16)
    from scipy.fftpack import dct
    x = np.random.default_rng(0).normal(size=(5, 40))
    np.testing.assert_allclose(np.dot(x, M.dct_rows().T.astype(float)), dct(x, type=2, axis=1, norm="ortho")[:, 1:14], rtol=0, atol=1e-13)


def test_reference_against_the_reference_projects_output():
    g = load_golden("G15_mfcc")
    worst = 0.0
    for i in range(int(g["n"])):
        fb, mf = M.mfcc_features_ref(g["signal%d" % i], int(g["rate%d" % i]))
        worst = max(worst, assert_close(fb, g["fbank%d" % i], "G15 fbank %d" % i), assert_close(mf, g["mfcc%d" % i], "G15 mfcc %d" % i))
    print("G15: largest deviation %.3g" % worst)
    assert worst < 1e-11, worst


@pytest.mark.parametrize("geo", M.GEOMETRIES + [M.DEFAULT], ids=lambda g: g[0])
def test_reference_against_the_oracle_on_every_geometry(geo):
    name, rate, fs, st, lo, hi, flen, step = geo
    assert M.frame_geometry(rate, fs, st) == (flen, step) == (int(fs * rate), int(st * rate))
    sigs = M.sweep_signals(geo)
    counts = [M.frame_count(len(x), step) for x in sigs]
    assert all(1500 <= len(x) <= 4000 for x in sigs)
    assert sum(counts) % 8 != 0 and any(c % 2 for c in counts)        # a last block with dead waves; changing partners
    worst = 0.0
    for x, T in zip(sigs, counts):
        fb, mf = M.mfcc_features_ref(x, rate, fs, st, lo, hi)
        ofb, omf = O.mfcc_features_signal(x, rate, fs, st, lo, hi)
        assert fb.shape == (T, 40) and mf.shape == (T, 13)
        worst = max(worst, assert_close(fb, ofb, name + " fbank"), assert_close(mf, omf, name + " mfcc"))
        # every bin carries energy, so log10(eps) stands exactly in the columns of the filters without a non-zero weight
        # (the rising half gives its first bin the weight 0, so a filter on the points (b, b + 1, b + 1) is empty too)
        empty = ~np.any(M.mel_filterbank(rate, lo, hi) != 0, axis=1)
        np.testing.assert_array_equal(fb == M.LOG_EPS, np.broadcast_to(empty, fb.shape))
        np.testing.assert_array_equal(ofb == M.LOG_EPS, np.broadcast_to(empty, fb.shape))
        assert empty.any() == (name in ("80-400", "80-1000")) and not empty.all()
    print("%s: largest deviation from the oracle %.3g" % (name, worst))
    assert worst < 1e-11, worst


def test_the_bands_are_what_the_sweep_says():
    by = {g[0]: g for g in M.GEOMETRIES}
    bins = lambda name: M.mel_bins(by[name][1], by[name][4], by[name][5])
    assert bins("44100")[0] == 0 and bins("low0")[0] == 0
    b = bins("80-1000")
    assert int(np.sum(np.diff(b) == 0)) == 11 and not np.any((b[2:] - b[:-2]) == 0)   # zero-width segments, no zero-width filter
    b = bins("80-400")
    assert b[0] == 2 and b[-1] == 12 and np.any((b[2:] - b[:-2]) == 0)
    assert bins("80-8016")[-1] == 257
    with pytest.raises(IndexError):                                    # bin 258: the reference indexes fbank[m - 1, 257]
        assert M.mel_bins(16000, 80, 8050)[-1] == 258
        M.mel_filterbank(16000, 80, 8050)
    assert M.frame_geometry(16000, 513.5 / 16000, 0.01)[0] == 513
    assert M.frame_geometry(16000, 0.025, 1e-5)[1] == 0


@pytest.mark.parametrize("geo", [M.DEFAULT, M.GEOMETRIES[0], M.GEOMETRIES[2]], ids=lambda g: g[0])
def test_length_edges(geo):
    name, rate, fs, st, lo, hi, flen, step = geo
    sigs = M.edge_signals(geo)
    assert [len(x) for x in sigs] == [1, step - 1, step, step + 1, flen - 1, flen, flen + 1]
    counts = [M.frame_count(len(x), step) for x in sigs]
    if name == "default":
        assert counts == [1, 1, 1, 2, 3, 3, 3]
    for x, T in zip(sigs, counts):
        fb, mf = M.mfcc_features_ref(x, rate, fs, st, lo, hi)
        ofb, omf = O.mfcc_features_signal(x, rate, fs, st, lo, hi)
        assert fb.shape == (T, 40)
        assert_close(fb, ofb, name + " fbank")
        assert_close(mf, omf, name + " mfcc")


def test_silent_cases_have_silent_rows_in_both_slots():
    want = {"a": [list(range(1, 13))], "b": [[0], [1]], "c": [[5, 6, 7, 8]], "d": [[], [0, 1, 2, 3, 4], []]}
    for name, sigs in M.silent_cases().items():
        slots = set()
        for x, rows in zip(sigs, want[name]):
            fb, mf = M.mfcc_features_ref(x, 16000)
            ofb, omf = O.mfcc_features_signal(x, 16000)
            quiet = M.silent_rows(fb)
            assert np.flatnonzero(quiet).tolist() == rows, name
            np.testing.assert_array_equal(ofb[quiet], M.LOG_EPS)       # the oracle's rows are exactly log10(eps) too
            assert not (fb[~quiet] == M.LOG_EPS).any()
            assert_close(fb, ofb, name)
            assert_close(mf, omf, name)
            slots |= {int(t) % 2 for t in np.flatnonzero(quiet)}       # frames pair (2m, 2m + 1) inside the utterance
        assert slots == {0, 1}, name                                   # a silent row in an A slot and one in a B slot
    d = M.silent_cases()["d"]
    assert [M.frame_count(len(x), 160) for x in d] == [13, 5, 11]      # odd counts: batch-wide pairs would cross utterances


def test_quiet_beside_loud_alternates_exactly():
    geo = M.GEOMETRIES[2]
    for first_loud, x in enumerate(M.quiet_loud_signals()):
        e = M.pre_emphasis(x).astype(float)
        peak = np.array([np.max(np.abs(e[256 * t:256 * (t + 1)])) for t in range(12)])
        loud = np.arange(12) % 2 == first_loud
        assert np.all(peak[loud] > 30000) and np.all(peak[~loud] <= 1.97) and np.all(peak[~loud] > 0)
        fb, mf = M.mfcc_features_ref(x, geo[1], *M.params(geo))
        ofb, omf = O.mfcc_features_signal(x, geo[1], *M.params(geo))
        assert fb.shape == (12, 40) and not (fb == M.LOG_EPS).any()
        assert np.all(np.min(fb[loud], axis=0) - np.max(fb[~loud], axis=0) > 7)    # filter by filter, seven decades between partners
        assert_close(fb, ofb, "quiet / loud fbank")
        assert_close(mf, omf, "quiet / loud mfcc")


def test_position_signals_have_the_frame_counts():
    assert [M.frame_count(len(x), 160) for x in M.position_signals()] == [3, 26, 5, 12]


def test_closed_forms_agree_with_the_dft():
    geo = M.GEOMETRIES[0]
    assert geo[6:] == (512, 160)
    for name, (x, power) in M.closed_form_cases().items():
        fb, mf = M.finish(power, geo[1], geo[4], geo[5])
        rfb, rmf = M.mfcc_features_ref(x, geo[1], *M.params(geo))
        dev = max(assert_close(fb, rfb, name), assert_close(mf, rmf, name))
        print("%s: closed form against the DFT %.3g" % (name, dev))
        quiet = M.silent_rows(fb)
        np.testing.assert_array_equal(quiet, M.silent_rows(rfb))
        if name.startswith("impulse"):
            s = int(name.split()[-1])
            held = [t for t in range(fb.shape[0]) if t * 160 <= s + 1 and s < t * 160 + 512]
            assert np.flatnonzero(~quiet).tolist() == held and {t % 2 for t in held} == {0, 1}
            assert {t % 2 for t in np.flatnonzero(quiet)} == {0, 1}    # silent rows beside them, in both slots
        else:
            assert not quiet.any()
        if name == "alternating":
            assert np.all(np.argmax(power, axis=1) == 256)
        if name == "constant":
            assert np.all(np.argmax(power, axis=1) == 0)
