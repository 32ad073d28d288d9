# -*- coding: utf-8 -*-
"""Bigram language model over word indices (the reference's sr/langmodel/langmodel.py is an empty file).

`BigramModel` counts sentence starts and adjacent word pairs in label strings -- the `label_seqs` that
`continuous_train` takes -- and turns them into the costs `-scale * log p` that the bigram grammar of the continuous
decoder adds (`sr.recognition.continuous_speech.build_bigram_grammar`, `ContinuousDecoder(grammar="bigram")`):
`init[w]` for starting with word w, `B[v, w]` for word w following word v.  Host side only; the decode with these costs
runs in the HIP kernels of libgmmhmm.so."""
import numpy as np

__all__ = ["BigramModel"]


class BigramModel:
    """Add-`smoothing` bigram estimates over `n_words` words.

        p(w | start) = (starts[w] + s) / (sum(starts) + s * n_words)
        p(w | v)     = (pairs[v, w] + s) / (sum(pairs[v]) + s * n_words)

    With `smoothing=0` an unseen start or pair has probability 0, i.e. cost +inf: the decoder cannot take it (the
    grammar builders leave the arc out); a word that was never followed by anything then forbids every successor."""

    def __init__(self, n_words, smoothing=1.0):
        n_words = int(n_words)
        smoothing = float(smoothing)
        if n_words < 1:
            raise ValueError("n_words must be at least 1, not %d" % n_words)
        if not smoothing >= 0.0 or np.isinf(smoothing):
            raise ValueError("smoothing must be a finite number >= 0, not %r" % (smoothing,))
        self.n_words = n_words
        self.smoothing = smoothing
        self.start_counts = np.zeros(n_words, dtype=np.float64)
        self.pair_counts = np.zeros((n_words, n_words), dtype=np.float64)

    def _labels(self, labels):
        a = np.asarray(labels)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError("a label string must be a flat sequence of word indices, not %r" % (labels,))
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.n_words):
            raise ValueError("word index out of range [0, %d) in %r" % (self.n_words, list(labels)))
        return a

    def fit(self, label_seqs):
        """Count sentence starts and adjacent pairs of `label_seqs` (replacing earlier counts); empty strings count
        nothing, a corpus without any word is an error.  Returns self."""
        starts = np.zeros(self.n_words, dtype=np.float64)
        pairs = np.zeros((self.n_words, self.n_words), dtype=np.float64)
        for labels in label_seqs:
            a = self._labels(labels)
            if a.size == 0:
                continue
            starts[a[0]] += 1
            np.add.at(pairs, (a[:-1], a[1:]), 1)
        if starts.sum() == 0:
            raise ValueError("cannot fit a bigram model on an empty corpus")
        self.start_counts, self.pair_counts = starts, pairs
        return self

    @staticmethod
    def _neg_log(num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
            return -np.log(p)

    def costs(self, scale=1.0):
        """(init [W], B [W, W]) in float64: -scale * log p; +inf where p = 0."""
        if self.start_counts.sum() == 0:
            raise ValueError("the model has not been fitted")
        scale = float(scale)
        if not scale > 0.0 or np.isinf(scale):
            raise ValueError("scale must be a finite number > 0, not %r" % (scale,))
        s, W = self.smoothing, self.n_words
        init = self._neg_log(self.start_counts + s, np.full(W, self.start_counts.sum() + s * W))
        B = self._neg_log(self.pair_counts + s, np.repeat(self.pair_counts.sum(axis=1, keepdims=True) + s * W, W, axis=1))
        return init * scale, B * scale

    def score(self, labels, scale=1.0):
        """Language-model cost of one word string: init[l0] + sum B[l_i, l_i+1] -- what the bigram grammar adds to the
        acoustic cost of a decode that returns `labels`.  0 for the empty string."""
        a = self._labels(labels)
        if a.size == 0:
            return 0.0
        init, B = self.costs(scale)
        return float(init[a[0]] + B[a[:-1], a[1:]].sum())

    def save(self, path):
        """Counts and smoothing as plain arrays (.npz)."""
        with open(path, "wb") as f:      # (a file object: np.savez would append ".npz" to a bare name)
            np.savez(f, n_words=np.array(self.n_words), smoothing=np.array(self.smoothing),
                     start_counts=self.start_counts, pair_counts=self.pair_counts)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            m = cls(int(z["n_words"]), float(z["smoothing"]))
            starts, pairs = np.array(z["start_counts"], dtype=np.float64), np.array(z["pair_counts"], dtype=np.float64)
        if starts.shape != (m.n_words,) or pairs.shape != (m.n_words, m.n_words) or (starts < 0).any() or (pairs < 0).any():
            raise ValueError("%s does not hold the counts of a %d-word bigram model" % (path, m.n_words))
        m.start_counts, m.pair_counts = starts, pairs
        return m
