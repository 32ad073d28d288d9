#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""Timing of sr.langmodel on the GPU (dict1 from tests/golden/G18_lextree.npz):
  long   text_viterbi of one seeded ~2 000-character typo text, end to end (flattening, upload, encode, kernels, join)
  batch  SpellChecker.spell_check of N dictionary words with random typos (tree resident: one upload at fit)
Prints one JSON line.   python tools/time_spellcheck.py [--batch 10000] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-recognition_amd"))


def typo(rng, w):
    letters = "abcdefghijklmnopqrstuvwxyz"
    w = list(w)
    for _ in range(int(rng.integers(0, 3))):
        k = int(rng.integers(len(w)))
        op = int(rng.integers(4))
        if op == 0:
            w[k] = letters[int(rng.integers(26))]
        elif op == 1 and len(w) > 1:
            del w[k]
        elif op == 2:
            w.insert(k, letters[int(rng.integers(26))])
        elif op == 3 and k + 1 < len(w):
            w[k], w[k + 1] = w[k + 1], w[k]
    return "".join(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chars", type=int, default=2000)
    args = ap.parse_args()
    from sr.langmodel import lextree_from_words, text_viterbi, SpellChecker
    from sr.langmodel.spellchecker import FlatTree
    words = [str(w) for w in np.load(os.path.join(ROOT, "tests", "golden", "G18_lextree.npz"))["words0"]]
    rng = np.random.default_rng(1)
    text, n = [], 0
    while n < args.chars:
        text.append(typo(rng, words[int(rng.integers(len(words)))]))
        n += len(text[-1]) + 1
    text = " ".join(text)[: args.chars]
    tree = lextree_from_words(list(words))
    R = FlatTree(tree).R
    text_viterbi("warm up", tree)
    long_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        text_viterbi(text, tree)
        long_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    sc = SpellChecker(beam=0)
    sc.fit(words)
    fit_ms = (time.perf_counter() - t0) * 1e3
    batch = [typo(rng, words[int(rng.integers(len(words)))]) for _ in range(args.batch)]
    cells = sum((len(x) + 1) * R for x in batch)
    sc.spell_check(batch[:64])
    batch_s = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        sc.spell_check(batch)
        batch_s.append(time.perf_counter() - t0)
    print(json.dumps(dict(rows=R, long_chars=len(text), long_ms_median=float(np.median(long_ms)), long_ms=long_ms,
                          fit_ms=fit_ms, batch=args.batch, batch_cells=cells, batch_s_median=float(np.median(batch_s)),
                          batch_cells_per_s=cells / float(np.median(batch_s)))))


if __name__ == "__main__":
    main()
