# -*- coding: utf-8 -*-
"""Batched drivers on top of the HIP kernels -- the call patterns of the reference's
`sr/core.py:test` (isolated-word arg-min over models, core.py:63-94) and `main.py`
(continuous-digit decode through a K-layer lattice + path post-processing,
main.py:35,59-67), over whole utterance batches resident in HBM.

These are what the benchmark and a serving caller use; the per-utterance functions
in `decode.py` give the same numbers one utterance at a time.
"""
import numpy as np

from . import _hip
from . import _pack
from .continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice

__all__ = ["IsolatedWordRecognizer", "ContinuousDecoder", "OnlineDecoder", "OnlineWordRecognizer", "InFlight", "path_to_words", "path_to_word_times", "word_spans",
           "sequence_report", "train_words", "vocabulary_posteriors"]


def _stack_models(ctx, models):
    """(states per word, packed Gaussians of all words, single-Gaussian flag).  A model trained with use_gmm=False has no
    `gmm_states` (hmm.py:57-76): its states are the rows of `mu` / `sigma`, scored by mahalanobis() (hmm.py:133-134)."""
    single = [not getattr(m, "use_gmm", True) or m.gmm_states is None for m in models]
    assert all(single) or not any(single), "word models with and without mixtures cannot share one recogniser"
    if single[0]:
        n = len(models[0].mu)
        for m in models:
            assert len(m.mu) == n
        mean = np.concatenate([np.asarray(m.mu, dtype=np.float64) for m in models])[:, None, :]
        var = np.concatenate([np.asarray(m.sigma, dtype=np.float64) for m in models])[:, None, :]
        key = (id(ctx), _pack._digest(mean, var, np.zeros(1)))
        gmm = _pack._gmm_cache.lookup(key, lambda: _hip.PackedGMM(ctx, mean, var, np.ones((len(mean), 1))))
        return n, gmm, True
    n = len(models[0].gmm_states)
    for m in models:
        assert len(m.gmm_states) == n
    return n, _pack.device_gmm(ctx, [s for m in models for s in m.gmm_states]), False


def train_words(templates_by_word, n_segments, n_gaussians=4, use_gmm=True, use_em=True):
    """`HMM(n_segments).fit(ys, n_gaussians, use_gmm, use_em)` for every word -- what sr/core.py:47-60 (make_HMM /
    train) does digit after digit -- in ONE pass over all words:

      1. segmental k-means of all words in lock-step (`kmeans.skmeans_multi`: one alignment launch and one
         (word, segment) reduction per iteration for all templates of all words),
      2. the mixtures of all W x n states refit in one lock-step session (`lockstep.LockstepFitter`; numpy's global
         generator is consumed word after word, state after state -- the order of the sequential loop),
      3. all templates re-aligned against their word's mixtures in one launch (align_gmm_states, hmm.py:95).

    templates_by_word: list over words of lists of [T_r, D] arrays.  Returns the list of trained `HMM`s; under the same
    numpy seed they equal the models of the word-after-word loop (alignment paths and cluster ids exactly, parameters to
    rounding: the words only share launches)."""
    import importlib
    _km = importlib.import_module(__package__ + ".kmeans")    # (the package re-exports the FUNCTION kmeans under that name)
    from .hmm import HMM
    from .hmm_state import GMM
    from .lockstep import LockstepFitter
    import os
    import sys
    import time
    marks = [("start", time.perf_counter())] if os.environ.get("GMMHMM_TRAIN_WORDS_TIMES") else None

    def mark(name):
        if marks is not None:
            marks.append((name, time.perf_counter()))
    W = len(templates_by_word)
    models = [HMM(n_segments) for _ in range(W)]
    for h in models:
        h.use_gmm, h.use_em = use_gmm, use_em
    if use_gmm:
        print('Doing segmental k-means')
    n = n_segments
    kmax = 2 ** max(1, int(np.log(n_gaussians)))
    on_device = bool(W) and all(len(ts) for ts in templates_by_word) and _km._device_skmeans_possible(templates_by_word[0]) and 2 <= n <= 32
    if not on_device:
        return _train_words_by_segments(templates_by_word, models, n, n_gaussians, use_gmm, use_em)
    # ONE resident batch of all templates for the three stages (round 4 uploaded the frames three times and regrouped them
    # on the host twice: 28 of the 50 ms of ten words x 200 templates)
    ctx = _hip.default_context()
    n_temps = np.array([len(ts) for ts in templates_by_word], dtype=np.int64)
    lengths = np.array([len(t) for ts in templates_by_word for t in ts], dtype=np.int64)
    D = np.asarray(templates_by_word[0][0]).shape[1]
    X, release = _km.host_workspace((int(lengths.sum()), D))
    try:
        _km.concat_rows([t for ts in templates_by_word for t in ts], X)
    except BaseException:
        release()
        raise
    off_t = np.concatenate([[0], np.cumsum(lengths)])
    mark("concatenate")
    try:
        return _train_words_resident(ctx, X, off_t, templates_by_word, models, n, n_gaussians, use_gmm, use_em, kmax, lengths, n_temps, mark, marks)
    finally:
        release()


def _train_words_resident(ctx, X, off_t, templates_by_word, models, n, n_gaussians, use_gmm, use_em, kmax, lengths, n_temps, mark, marks):
    """The three stages of `train_words` on ONE resident batch of all templates (X: the caller's frames back to back)."""
    import importlib
    import sys
    _km = importlib.import_module(__package__ + ".kmeans")
    from .hmm_state import GMM
    from .lockstep import LockstepFitter
    W, D = len(templates_by_word), X.shape[1]
    frames = _hip.Batch(ctx, feats=X, offsets=off_t)
    mark("upload")
    try:
        fitted = _km.skmeans_multi(templates_by_word, n, frames=frames)
        mark("segmental k-means")
        tpl_off = np.concatenate([[0], np.cumsum(n_temps)])
        for w, h in enumerate(models):
            h.mu, h.sigma, h.transitions, _ = fitted[w]
        starts = np.concatenate([f[3] for f in fitted])
        order, counts = _km.segment_order(lengths, n_temps, starts, n)
        if not use_gmm:
            for h, segs in zip(models, _km.split_segments(_km.gather_rows(X, order), counts)):
                h.segments = segs
            return models
        for h in models:
            h.gmm_states = [GMM(m, s, n_gaussians) for m, s in zip(h.mu, h.sigma)]
        mark("segment order, GMM objects")
        # the mixtures of all W x n states: their frames gathered on the device from the resident batch
        fitter = LockstepFitter(None, ctx=ctx, source=(frames, order), lengths=[int(c) for c in counts.reshape(-1)], dim=D, kmax=kmax)
        try:
            fitter.split_and_fit([g for h in models for g in h.gmm_states],
                                 start_centroids=np.concatenate([h.mu for h in models]),
                                 weight_divisor=[int(c) for c in counts.reshape(-1)],     # hmm.py:108,118: len(segment)
                                 n_gaussians=n_gaussians, use_em=use_em)
        finally:
            fitter.close()
        mark("refit")
        # re-alignment of every template against its word's mixtures (hmm.py:95), all words in one launch
        utt_word = np.repeat(np.arange(W), n_temps).astype(np.int32)
        gmm = _pack.device_gmm(ctx, [g for h in models for g in h.gmm_states])
        lat = _hip.Lattices(ctx, [_pack.graph_from_dense(np.arange(n) + w * n, h.transitions, [0], [n - 1]) for w, h in enumerate(models)])
        try:
            frames.loglik(gmm, fetch=False, state_ranges=(utt_word * n, utt_word * n + n))
            res = lat.viterbi(frames, utt_lattice=utt_word, want_path=True, flat_paths=True)
        finally:
            lat.close()
        mark("re-alignment")
    finally:
        frames.close()
    # get_segments_from_path for all templates at once: visits of every chain row on the path, cumulated (kmeans.py:98-108)
    tid = np.repeat(np.arange(len(lengths)), res["path_len"])
    visits = np.bincount(tid * n + res["path_flat"][:, 0], minlength=len(lengths) * n).reshape(len(lengths), n)
    starts_all = np.zeros((len(lengths), n), dtype=np.int64)
    np.cumsum(visits[:, :-1], axis=1, out=starts_all[:, 1:])
    order, counts = _km.segment_order(lengths, n_temps, starts_all, n)
    mark("segment order")
    for h, segs in zip(models, _km.split_segments(_km.gather_rows(X, order), counts)):
        h.segments = segs
    mark("segments")
    if marks is not None:
        sys.stderr.write("train_words [ms]: " + ", ".join("%s %.2f" % (b[0], (b[1] - a[1]) * 1e3) for a, b in zip(marks, marks[1:])) + "\n")
    return models


def _starts_from_paths(paths, n):
    """get_segments_from_path for all templates at once: visits of every chain row on the path, cumulated (kmeans.py:98-108)."""
    plen = np.array([len(p) for p in paths], dtype=np.int64)
    rows = (np.concatenate([np.asarray(p)[:, 0] for p in paths]) if len(paths) and plen.sum() else np.zeros(0, dtype=np.int64)).astype(np.int64)
    tid = np.repeat(np.arange(len(paths)), plen)
    counts = np.bincount(tid * n + rows, minlength=len(paths) * n).reshape(len(paths), n)   # (rows: chain rows 0 .. n-1 of the word's own graph)
    starts_all = np.zeros((len(paths), n), dtype=np.int64)
    np.cumsum(counts[:, :-1], axis=1, out=starts_all[:, 1:])
    return starts_all


def _train_words_by_segments(templates_by_word, models, n_segments, n_gaussians, use_gmm, use_em):
    """train_words with the frames regrouped on the host (one feature dimension, word lists with an empty entry, the test
    double of the binding): the stages of `HMM.fit`, the refit and the re-alignment still one launch sequence for all words."""
    import importlib
    _km = importlib.import_module(__package__ + ".kmeans")
    from .hmm_state import GMM
    from .lockstep import LockstepFitter
    W = len(templates_by_word)
    for w, h in enumerate(models):
        h.mu, h.sigma, h.transitions, h.segments = _km.skmeans(templates_by_word[w], n_segments, return_segmented_data=True)
    if not use_gmm:
        return models
    for h in models:
        h.gmm_states = [GMM(m, s, n_gaussians) for m, s in zip(h.mu, h.sigma)]
    fitter = LockstepFitter([seg for h in models for seg in h.segments], kmax=2 ** max(1, int(np.log(n_gaussians))))
    try:
        fitter.split_and_fit([g for h in models for g in h.gmm_states],
                             start_centroids=np.concatenate([h.mu for h in models]),
                             weight_divisor=[len(seg) for h in models for seg in h.segments],     # hmm.py:108,118
                             n_gaussians=n_gaussians, use_em=use_em)
    finally:
        fitter.close()
    ctx = _hip.default_context()
    flat = [np.asarray(t, dtype=np.float64) for ts in templates_by_word for t in ts]
    utt_word = np.repeat(np.arange(W), [len(ts) for ts in templates_by_word]).astype(np.int32)
    n = n_segments
    gmm = _pack.device_gmm(ctx, [g for h in models for g in h.gmm_states])
    lat = _hip.Lattices(ctx, [_pack.graph_from_dense(np.arange(n) + w * n, h.transitions, [0], [n - 1]) for w, h in enumerate(models)])
    frames = _hip.Batch(ctx, flat)
    try:
        frames.loglik(gmm, fetch=False, state_ranges=(utt_word * n, utt_word * n + n))
        res = lat.viterbi(frames, utt_lattice=utt_word, want_path=True)
    finally:
        frames.close()
        lat.close()
    off = np.concatenate([[0], np.cumsum([len(ts) for ts in templates_by_word])])
    starts_all = _starts_from_paths(res["paths"], n)
    for w, h in enumerate(models):
        h.segments = _km.segment_data_fast(templates_by_word[w], n, starts_all[off[w]:off[w + 1]])
    return models


def _posterior_args(W, scale, log_prior):
    """(scale, log_prior [W]) checked: scale finite and > 0; log_prior None (zeros) or W values, each finite or -inf."""
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        raise ValueError("scale must be a finite number > 0")
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError("scale must be a finite number > 0, not %r" % scale)
    if log_prior is None:
        return scale, np.zeros(W, dtype=np.float64)
    lp = np.asarray(log_prior, dtype=np.float64)
    if lp.shape != (W,):
        raise ValueError("log_prior must hold one value per word (%d), not shape %r" % (W, lp.shape))
    if np.any(np.isnan(lp)) or np.any(np.isposinf(lp)):
        raise ValueError("every log_prior must be finite or -inf")
    return scale, lp


def vocabulary_posteriors(soft, scale=1.0, log_prior=None):
    """The posterior over the vocabulary from soft costs [U, W] (soft[u, w] = -log P(x_u | w), +inf: no path): with
    z[w] = scale * soft[u, w] - log_prior[w] and m = min_w z, p[w] = exp(m - z[w]) and post[u, w] = p[w] / sum_w p, the sum
    taken in ascending w.  scale < 1 flattens the over-sharp acoustic scores; a word with log_prior -inf gets 0; a row
    whose z are all +inf is a row of zeros.  The ONE statement of the softmax: the one-shot and the online recogniser both
    call it, which makes their posteriors equal where their soft costs are."""
    soft = np.asarray(soft, dtype=np.float64)
    if soft.ndim != 2:
        raise ValueError("soft costs are a [U, W] matrix")
    U, W = soft.shape
    scale, lp = _posterior_args(W, scale, log_prior)
    post = np.zeros((U, W), dtype=np.float64)
    if U == 0 or W == 0:
        return post
    with np.errstate(invalid="ignore"):
        z = scale * soft - lp[None, :]
    z[np.isnan(z)] = np.inf                               # (no path and no prior: still no word)
    m = z.min(axis=1)
    live = np.flatnonzero(np.isfinite(m))
    if not len(live):
        return post
    p = np.exp(m[live, None] - z[live])
    s = np.zeros(len(live), dtype=np.float64)
    for w in range(W):                                    # ascending w: the order is part of the definition
        s = s + p[:, w]
    post[live] = p / s[:, None]
    return post


def _posterior_info(soft, words, scale, log_prior):
    """The four keys a recogniser adds: soft_costs, posteriors, confidence = post[u, words[u]] (0.0 for a zero row or no
    word) and soft_words, the first arg-max of every row (-1 for a zero row)."""
    post = vocabulary_posteriors(soft, scale, log_prior)
    words = np.asarray(words, dtype=np.int64)
    U = len(words)
    any_ = post.any(axis=1) if post.shape[1] else np.zeros(U, dtype=bool)
    soft_words = np.where(any_, np.argmax(post, axis=1) if post.shape[1] else 0, -1).astype(np.int64)
    conf = np.zeros(U, dtype=np.float64)
    ok = words >= 0
    conf[ok] = post[np.flatnonzero(ok), words[ok]]
    return dict(soft_costs=soft, posteriors=post, confidence=conf, soft_words=soft_words)


class IsolatedWordRecognizer:
    """Scores every utterance against every word model and returns the arg-min word
    (core.py:82-87: `costs = [m.evaluate(x) for m in models]; argmin`).

    The W word chains are stacked into one graph (W start rows, W end rows), so one
    gh_loglik + one gh_viterbi launch replaces U x W calls of HMM.evaluate.

    POSTERIORS (not in the reference).  `soft_costs` gives -log P(x | w) summed over all paths of every
    word (the forward sweep, gh_chain_forward), `posteriors` the softmax of them over the vocabulary
    (`vocabulary_posteriors`), and `recognize(want_posteriors=True)` the confidence of the arg-min word, with
    `min_confidence=` as a rejection threshold (word -1).  Single-Gaussian recognisers (one Gaussian per state: scored
    inside the fused sweep, no likelihood matrix exists) raise `_hip.Unsupported`."""

    def __init__(self, models, device=None, dtype=np.float64, ctx=None):
        self.ctx = ctx if ctx is not None else _hip.default_context(device)
        self.dtype = dtype
        self.W = len(models)
        self.n, self.gmm, self.single = _stack_models(self.ctx, models)
        n, W = self.n, self.W
        to, frm, cost = [], [], []
        for i, m in enumerate(models):
            t = np.asarray(m.transitions, dtype=np.float64)
            a, b = np.nonzero(~np.isinf(t))
            to.append(a + i * n)
            frm.append(b + i * n)
            cost.append(t[a, b])
        graph = dict(row_state=np.arange(W * n, dtype=np.int32), arc_to=np.concatenate(to),
                     arc_from=np.concatenate(frm), arc_cost=np.concatenate(cost),
                     start_rows=np.arange(W) * n, end_rows=np.arange(W) * n + n - 1)
        self.lat = _hip.Lattices(self.ctx, [graph])

    def costs(self, batch):
        """[U, W] matrix of HMM.evaluate values for a resident `_hip.Batch`.  Models with ONE Gaussian per state
        (use_gmm=False, or one-component mixtures) are scored inside the dynamic program -- the reference's own
        single-Gaussian path, hmm.py:133-134 (`dtw` with `mahalanobis`): no [N, S] likelihood matrix exists
        (gh_viterbi_fused); mixtures run gh_loglik + gh_viterbi."""
        if self.gmm.M == 1:
            r = self.lat.viterbi(batch, want_path=False, fused_gmm=self.gmm, log_domain=self.single)
        else:
            batch.loglik(self.gmm, fetch=False)
            r = self.lat.viterbi(batch, want_path=False)
        return r["end_cost_flat"].reshape(batch.U, self.W)

    def _refuse_single(self, what):
        if self.gmm.M == 1:
            raise _hip.Unsupported("%s need the likelihood matrix: a recogniser with one Gaussian per state is scored inside the "
                                   "fused sweep, which has no forward form" % what)

    def soft_costs(self, batch):
        """[U, W] matrix of -log P(x_u | word w), summed over ALL paths of the word's chain (the forward sweep on the
        resident likelihood matrix, computed here when the batch holds none); +inf where a word has no path."""
        self._refuse_single("soft costs")
        if batch.S is None:
            batch.loglik(self.gmm, fetch=False)
        return self.lat.chain_forward(batch).reshape(batch.U, self.W)

    def posteriors(self, batch, scale=1.0, log_prior=None):
        """(post [U, W], soft [U, W]): `vocabulary_posteriors` of `soft_costs(batch)`."""
        self._refuse_single("posteriors")
        _posterior_args(self.W, scale, log_prior)
        soft = self.soft_costs(batch)
        return vocabulary_posteriors(soft, scale, log_prior), soft

    def recognize(self, xs, want_posteriors=False, scale=1.0, log_prior=None, min_confidence=None):
        """xs: list of [T_u, D] arrays -> (words [U], costs [U, W]).  want_posteriors=True: (words, costs, info) with info =
        dict(soft_costs [U, W], posteriors [U, W], confidence [U] = posteriors[u, words[u]], soft_words [U]: the first
        arg-max of every row of the posteriors, -1 for a row of zeros); `words` stays the Viterbi arg-min.  min_confidence=c
        (needs want_posteriors) sets words[u] = -1 where the confidence is below c."""
        if not want_posteriors:
            if min_confidence is not None:
                raise ValueError("min_confidence needs want_posteriors=True")
        else:
            self._refuse_single("posteriors")
            _posterior_args(self.W, scale, log_prior)
            if min_confidence is not None and np.isnan(float(min_confidence)):
                raise ValueError("min_confidence must be a number")
        batch = _hip.Batch(self.ctx, xs, dtype=self.dtype)
        try:
            c = self.costs(batch)
            soft = self.soft_costs(batch) if want_posteriors else None
        finally:
            batch.close()
        words = np.argmin(c, axis=1)
        if not want_posteriors:
            return words, c
        info = _posterior_info(soft, words, scale, log_prior)
        if min_confidence is not None:
            words = np.where(info["confidence"] < float(min_confidence), -1, words)
        return words, c, info

    def accuracy(self, xs, words, verbose=False):
        """The report of `sr/core.py:test` (core.py:63-94) as a call: fraction of utterances whose cheapest model is
        the labelled word.  The reference keeps the FIRST of equal minima (`if cost < c`), which is np.argmin's rule.
        Returns (n_passed / n_tests, recognised words [U])."""
        got, _ = self.recognize(xs)
        words = np.asarray(words)
        if verbose:
            for w in words[got != words]:
                print("Digit:", int(w), "is wrong")                       # core.py:93
        return float(np.sum(got == words)) / len(words), got


    def online(self, n_streams, frontend=None, endpointer=None, soft=False, scale=1.0, log_prior=None):
        """An `OnlineWordRecognizer` of `n_streams` live utterances sharing this recogniser's packed mixtures and graph
        (single-Gaussian word models raise `_hip.Unsupported`).  frontend / endpointer: as `ContinuousDecoder.online` -- a
        `sr.feature.StreamingFrontend` (`push_audio`) and a `sr.audio_capture.StreamingEndpointer` (`push_recording`) of
        the same context and `n_streams`.  soft=True: the streams carry the forward column too, and `result` / `finish` /
        `push_recording` report posteriors and a confidence under `scale` and `log_prior` (as `recognize`)."""
        return OnlineWordRecognizer(self, n_streams, frontend, endpointer, soft=soft, scale=scale, log_prior=log_prior)


def sequence_report(decoded, labels, verbose=False):
    """The tally at the end of the reference's `main.py` (:69-84): an utterance is correct when its decoded word
    string equals the label string; for a wrong one the number of differing positions (np.count_nonzero(matched - l),
    strings of equal length -- the K-layer lattice always decodes exactly K words) counts against the digit accuracy.
    Returns dict(sequence_accuracy, digit_accuracy, n_correct, n_digits, n_digit_errors)."""
    correct = n_digits = n_diff = 0
    for got, want in zip(decoded, labels):
        got, want = [int(v) for v in got], [int(v) for v in want]
        n_digits += len(want)
        if got == want:
            correct += 1
            if verbose:
                print('Correct:', got)
            continue
        if verbose:
            print('Incorrect:', got, want)
        if len(got) != len(want):
            # main.py:79 subtracts the two arrays, which numpy refuses for different lengths (the loop grammar can
            # produce them): every position beyond the shorter string counts as a difference here
            k = min(len(got), len(want))
            d = int(np.count_nonzero(np.asarray(got[:k]) - np.asarray(want[:k]))) + max(len(got), len(want)) - k
        else:
            d = int(np.count_nonzero(np.asarray(got) - np.asarray(want)))
        if verbose:
            print('Diff:', d)
        n_diff += d
    n = max(len(labels), 1)
    return dict(sequence_accuracy=correct / n, digit_accuracy=(n_digits - n_diff) / max(n_digits, 1), n_correct=correct,
                n_digits=n_digits, n_digit_errors=n_diff)


def path_to_words(path, row_state, n_per_word):
    """main.py:59-67: reversed path rows -> drop consecutive duplicates -> first emitting
    row of every run between non-emitting rows -> word index of that row."""
    if len(path) == 0:
        return []
    rows = np.asarray(path)[:, 0][::-1]
    rows = rows[np.insert(np.diff(rows) != 0, 0, True)]
    st = np.asarray(row_state)[rows]
    emitting = st >= 0
    # first emitting row of each maximal emitting run
    first = emitting & np.insert(~emitting[:-1], 0, True)
    return [int(s) // n_per_word for s in st[first]]


def path_to_word_times(path, row_state, n_per_word):
    """(words, begins) of a path as decode_hmm_states returns it (end -> start, without the end cell) -- the host statement
    of the begin rule.  Walk the path start -> end (main.py:59-67): a word is a maximal run of cells on emitting rows
    between non-emitting rows, its label is the label of the run's first cell (`path_to_words`), and ITS BEGIN IS THE
    COLUMN OF THAT FIRST CELL.  Begins are frame indices inside the utterance; an empty path gives two empty lists."""
    if len(path) == 0:
        return [], []
    cells = np.asarray(path)[::-1]
    st = np.asarray(row_state)[cells[:, 0]]
    emitting = st >= 0
    first = emitting & np.insert(~emitting[:-1], 0, True)
    return [int(s) // n_per_word for s in st[first]], [int(c) for c in cells[first, 1]]


def word_spans(begins, frames):
    """[(begin, end), ...] of the words of one utterance of `frames` frames from their begins: word k ends where word
    k + 1 begins and the last word ends at the utterance's frame count.  (A non-emitting row shares its column with the
    cell behind it, so a word's last frame and the next word's first frame are the same column; like the regrouping of
    continuous_train, the boundary frame goes to the next word only.  The spans tile [begins[0], frames).)"""
    b = [int(x) for x in begins]
    return list(zip(b, b[1:] + [int(frames)]))


class ContinuousDecoder:
    """Continuous-word decode over all `models`, then `path_to_words`.

    grammar="layers": the reference's K-layer lattice (main.py:35: build_state_sequences(models,
    [[0..W-1]] * K)) -- exactly `n_layers` words; end points = last layer's final states in the last
    column (main.py:60).
    grammar="loop": the word-loop grammar (`build_loop_grammar`) -- any number of
    words, cost = min over K of the K-layer costs, on a graph of 2 + W*n rows instead of
    1 + K*(W*n + 1).
    grammar="bigram": the loop grammar with word-to-word costs (`build_bigram_grammar`): `bigram` is a [W, W] cost
    matrix (`bigram[v, w]`: word w after word v, +inf = forbidden) with optional start costs `initial` [W], or a
    `sr.langmodel.BigramModel`, whose `costs(lm_scale)` are then used.  Up to 16 words of 2..8, 12 or 16 states
    run on the bigram-form kernel, 17 to 64 words of 2..8 states on the wide one (a wave per utterance, lane = word);
    anything else decodes on the row-per-lane kernels, same results.  (`online_bigram` takes up to 16 words, and 17 to 64
    with `wide=True`.)"""

    def __init__(self, models, n_layers=7, device=None, dtype=np.float64, grammar="layers", word_penalty=0.0, ctx=None,
                 bigram=None, initial=None, lm_scale=1.0):
        self.ctx = ctx if ctx is not None else _hip.default_context(device)
        self.dtype = dtype
        # (single-Gaussian word models decode through the likelihood kernel here: mahalanobis() is the one-component
        #  GMM.evaluate with weight 1, the same number up to rounding)
        self.n, self.gmm, _ = _stack_models(self.ctx, models)
        W = len(models)
        wt = [m.transitions for m in models]
        if grammar == "layers":
            graph, self.nes_rows = packed_lattice(wt, self.n, [list(range(W))] * n_layers)
            self._max_labels = lambda T: n_layers + 1
        elif grammar == "loop":
            graph, self.nes_rows = packed_loop_lattice(wt, self.n, word_penalty)
            self._max_labels = lambda T: T // max(1, self.n - 1) + 2      # a word spans at least n - 1 column steps
        elif grammar == "bigram":
            if bigram is None:
                raise ValueError("grammar='bigram' needs `bigram`: a [W, W] cost matrix or a BigramModel")
            if hasattr(bigram, "costs"):
                if initial is not None:
                    raise ValueError("`initial` comes from the BigramModel; pass either a model or cost arrays")
                if bigram.n_words != W:
                    raise ValueError("the BigramModel has %d words, the decoder %d" % (bigram.n_words, W))
                initial, bigram = bigram.costs(lm_scale)
            graph, self.nes_rows = packed_bigram_lattice(wt, self.n, bigram, initial)
            self._max_labels = lambda T: T // max(1, self.n - 1) + 2      # as for the loop grammar
        else:
            raise ValueError("grammar must be 'layers', 'loop' or 'bigram', not %r" % (grammar,))
        self.grammar = grammar
        self.n_words = W
        self.n_layers = n_layers if grammar == "layers" else None
        self.row_state = graph["row_state"]
        self.lat = _hip.Lattices(self.ctx, [graph])

    def _posteriors_refusal(self, lm=False, layers=False):
        """Why this decoder has no word posteriors (None: it has).  Decided from what the decoder was built with, before the
        GPU is touched; the library refuses the same cases on its own.  lm=True permits the bigram grammar
        (gh_word_posteriors_bigram), layers=True the K-layer lattice (gh_word_posteriors_layers: 1 to 8 layers of up to 16
        words); without its keyword either decoder is refused as it always was."""
        if self.grammar == "bigram" and not lm:
            return ("word posteriors and confidences are built for the word-loop grammar (grammar='loop'); the bigram grammar "
                    "(one entry row per word) is not built")
        if self.grammar == "layers" and not layers:
            return ("word posteriors and confidences are built for the word-loop grammar (grammar='loop'); the K-layer lattice "
                    "is not built without layers=True")
        if self.grammar == "layers" and self.n_words > 16:
            return ("word posteriors on the K-layer lattice are built for up to 16 words per layer, not %d (the wide layer form)"
                    % self.n_words)
        if self.grammar == "layers" and self.n_layers > 8:
            return "word posteriors on the K-layer lattice are built for up to 8 layers, not %d" % self.n_layers
        if getattr(self.lat, "beam", 0):
            return ("word posteriors are sums over all paths: a decoder with a rank beam (set_beam(%d)) has none"
                    % self.lat.beam)
        if self.n > 8:
            return "word posteriors are built for words of 2 to 8 states, not %d" % self.n
        return None

    def _posteriors_call(self, lm, layers=False):
        """The backend method that computes this decoder's word posteriors: `word_posteriors_bigram` for a permitted bigram
        decoder, `word_posteriors_layers` for a permitted layers decoder, `word_posteriors` otherwise.  A one-word bigram
        grammar has the rows of the loop form; it goes by the form the library reports for its handle."""
        if self.grammar == "layers" and layers:
            return self.lat.word_posteriors_layers
        if self.grammar == "bigram" and lm and not (self.n_words == 1 and "loop" in self.lat.forms()):
            return self.lat.word_posteriors_bigram
        return self.lat.word_posteriors

    def word_posteriors(self, batch, lm=False, layers=False):
        """(post, logp): the word posteriorgram post [N, W] of the batch (row = frame in batch order, post[t, w] = the posterior
        that frame t belongs to word w -- a boundary frame belongs to the entering word, as in the begin times -- every row
        of an utterance with a path sums to 1) and log P [U] per utterance, from one forward-backward over the loop grammar
        (gh_word_posteriors).  grammar="loop" with words of 2 to 8 states and no beam; anything else raises `_hip.Unsupported`.
        lm=True is a permission, not a demand: a grammar="bigram" decoder (2 to 8 states, no beam) then answers too, from the
        forward-backward over the bigram grammar (gh_word_posteriors_bigram); nothing else changes.
        layers=True is the same kind of permission for a grammar="layers" decoder of 1 to 8 layers of up to 16 words (2 to 8
        states, no beam): post is summed over the layers (gh_word_posteriors_layers).  Loop and bigram decoders ignore it."""
        why = self._posteriors_refusal(lm, layers)
        if why:
            raise _hip.Unsupported(why)
        batch.loglik(self.gmm, fetch=False)
        r = self._posteriors_call(lm, layers)(batch)
        return r["post"], r["logp"]

    def decode_batch(self, batch, want_path=False, want_times=False, want_confidence=False, lm=False, layers=False):
        """Word-index lists of every utterance (+ the raw result dict).  By default the paths stay on the device
        and only the decoded word sequences come back (gh_viterbi_labels); want_path=True also returns the
        reference-style (row, column) paths in `r["paths"]` and derives the words from them on the host.
        want_times=True: `r["begins"]` holds one int32 array per utterance, aligned with its words -- the frame every word
        begins in (`path_to_word_times`; gh_viterbi_labels_timed, or the host rule on the paths with want_path=True).
        Word k ends where word k + 1 begins, the last one at the utterance's frame count (`word_spans`).
        want_confidence=True (grammar="loop", words of 2 to 8 states, no beam; else `_hip.Unsupported`): the decode of
        want_times=True, then one gh_word_posteriors call on the same likelihoods: `r["confidence"]` holds one float64 array
        per utterance, aligned with its words -- the mean over the word's frames of the posterior that the frame belongs to
        that word, in [0, 1] -- with `r["begins"]` and `r["logp"]` (log P per utterance).  Words, begins, end costs and
        chosen ends are those of want_times=True bit for bit.
        lm=True (with want_confidence=True; a permission, ignored otherwise): a grammar="bigram" decoder of 2 to 8 states
        without a beam is not refused -- the same decode, then one gh_word_posteriors_bigram call.
        layers=True (likewise a permission): a grammar="layers" decoder of 1 to 8 layers of up to 16 words of 2 to 8 states
        without a beam is not refused -- the same decode, then one gh_word_posteriors_layers call."""
        if want_confidence:
            why = self._posteriors_refusal(lm, layers)
            if why:
                raise _hip.Unsupported(why)
            if want_path:
                raise ValueError("want_confidence goes with the label decode, not with want_path")
            words, r = self.decode_batch(batch, want_times=True)
            wp = self._posteriors_call(lm, layers)(batch, labels=r["labels"], begins=r["begins"], want_post=False)
            r["confidence"], r["logp"] = wp["confidence"], wp["logp"]
            return words, r
        batch.loglik(self.gmm, fetch=False)
        if want_path:
            r = self.lat.viterbi(batch, want_path=True)
            if want_times:
                wt = [path_to_word_times(p, self.row_state, self.n) for p in r["paths"]]
                r["begins"] = [np.asarray(b, dtype=np.int32) for _, b in wt]
                return [w for w, _ in wt], r
            return [path_to_words(p, self.row_state, self.n) for p in r["paths"]], r
        row_word = np.where(self.row_state >= 0, self.row_state // self.n, -1).astype(np.int32)
        if want_times:
            r = self.lat.viterbi_labels(batch, row_word, max_labels=self._max_labels(batch.lengths), want_begin=True)
        else:
            r = self.lat.viterbi_labels(batch, row_word, max_labels=self._max_labels(batch.lengths))
        return [[int(w) for w in l] for l in r["labels"]], r

    def decode(self, xs, want_times=False, want_confidence=False, lm=False, layers=False):
        """xs: list of [T_u, D] arrays -> list of word-index lists; want_times=True: (words, begins), begins one int32
        array per utterance (see `decode_batch`); want_confidence=True: (words, begins, confidence), confidence one
        float64 array per utterance; lm=True permits that for a grammar="bigram" decoder, layers=True for a
        grammar="layers" decoder (see `decode_batch`)."""
        if want_confidence:
            why = self._posteriors_refusal(lm, layers)
            if why:
                raise _hip.Unsupported(why)
        batch = _hip.Batch(self.ctx, xs, dtype=self.dtype)
        try:
            if want_confidence:
                words, r = self.decode_batch(batch, want_confidence=True, lm=lm, layers=layers)
                return words, r["begins"], r["confidence"]
            if want_times:
                words, r = self.decode_batch(batch, want_times=True)
                return words, r["begins"]
            return self.decode_batch(batch)[0]
        finally:
            batch.close()

    def accuracy(self, xs, labels, verbose=False):
        """Decode `xs` and tally against the label strings like main.py:54-84 -- see `sequence_report`."""
        return sequence_report(self.decode(xs), labels, verbose=verbose)

    def online(self, n_streams, max_frames=None, window=None, frontend=None, endpointer=None, times=False, settle=False,
               max_tail=None):
        """An `OnlineDecoder` of `n_streams` live utterances sharing this decoder's packed mixtures and graph
        (grammar="loop" only: anything else raises `_hip.Unsupported`).  Exactly one of `max_frames` (utterances of up to
        that many frames, whole history kept) and `window` (utterances of any length, history for that many unsettled
        frames) must be given.  frontend: a `sr.feature.StreamingFrontend` of the same context, dtype and `n_streams`
        (39 features, like the models) -- the decoder then takes audio (`push_audio`).  endpointer: a
        `sr.audio_capture.StreamingEndpointer` of the same context, sample rate and `n_streams` (needs a front-end) -- the
        decoder then takes whole recordings and cuts the utterances out itself (`push_recording`).  times=True: the
        decoder also keeps and reports the frame every word begins in (see `OnlineDecoder`).  A decoder of more than 16
        words (up to 64, of 2..8 states) by default takes `max_frames` only, keeps its full history and does not settle;
        `settle=True` gives it the settled prefix (`commit`, `settled`, `settled_times`) with `max_frames=` and lets it
        take `window=`.  A decoder of up to 16 words always settles and ignores `settle`.  max_tail=M (a decoder of up to
        16 words; 1 <= M < window) makes `commit` a FORCED commit: afterwards a stream holds at most M unsettled frames,
        whether its traces met or not (see `OnlineDecoder`); with None nothing changes anywhere."""
        return OnlineDecoder(self, n_streams, max_frames, window, frontend, endpointer, times, settle, max_tail)


    def online_bigram(self, n_streams, max_frames=None, window=None, frontend=None, endpointer=None, times=False, settle=False,
                      wide=False):
        """An `OnlineBigramDecoder` of `n_streams` live utterances sharing this decoder's packed mixtures and bigram graph
        (grammar="bigram" only: anything else raises `_hip.Unsupported` before the GPU is touched).  Exactly one of
        `max_frames` (utterances of up to that many frames, whole history kept) and `window` (utterances of any length,
        history for that many unsettled frames) must be given.  The settled prefix (`commit`, `settled`,
        `settled_times`) is opt-in: `window=` implies it, `max_frames=..., settle=True` asks for it; without either the
        decoder refuses those three calls.  frontend / endpointer / times: as in `online`.  The language-model costs
        (`bigram`, `initial`, `lm_scale`) are in the graph; nothing is passed again.  wide=True lets a decoder of more
        than 16 words (up to 64, of 2..8 states) run on the wide bigram session: `max_frames` only, full history, nothing
        settles (`window=` and `settle=True` raise `_hip.Unsupported` before the GPU is touched).  wide="settle" lets it
        run there in all three forms -- `max_frames=`, `max_frames=..., settle=True` and `window=` -- with the settled
        prefix of a narrow bigram decoder.  Both are permissions, not demands: a decoder of up to 16 words is served as
        without them, and without them a larger decoder is refused as before.  Any other value of `wide` is a ValueError."""
        return OnlineBigramDecoder(self, n_streams, max_frames, window, frontend, endpointer, times, settle, wide)

    def online_layers(self, n_streams, max_frames, frontend=None, endpointer=None, times=False):
        """An `OnlineLayersDecoder` of `n_streams` live utterances sharing this decoder's packed mixtures and K-layer
        lattice (grammar="layers" only: anything else raises `_hip.Unsupported` before the GPU is touched).  `max_frames`
        is a hard capacity per stream: an utterance of exactly `n_layers` words is bounded in length, so the whole
        history is kept, nothing settles (`commit`, `settled` and `settled_times` raise `_hip.Unsupported`) and there is
        no window.  frontend / endpointer / times: as in `online`.  Taken: 1 to 8 layers of up to 16 words of 2 to 8
        states; 9 to 16 layers, words of 12 or 16 states and 17 to 64 words are not offered yet (`_hip.Unsupported`)."""
        return OnlineLayersDecoder(self, n_streams, max_frames, frontend, endpointer, times)


class _OnlineStreams:
    """The stream plumbing `OnlineDecoder` and `OnlineWordRecognizer` share: `n_streams` live utterances that take feature
    frames (`push`, `push_batch`), audio through a `StreamingFrontend` (`push_audio`) or recordings through a
    `StreamingEndpointer` as well (the gate loop of `push_recording`), with every argument checked on the host first.
    A subclass provides `self.session` (`push(batch, ids, first, count)`, `reset(ids)`), `_room(ids, counts)` (raises
    ValueError where the streams cannot take that many frames) and `result`."""

    _what = "decoder"

    def _attach(self, ctx, dtype, gmm, n_streams, frontend, endpointer):
        what = self._what
        if frontend is not None:
            if frontend.ctx is not ctx:
                raise ValueError("the front-end lives on another context than the %s" % what)
            if np.dtype(frontend.dtype) != np.dtype(dtype):
                raise ValueError("the front-end emits %s, the %s takes %s" % (np.dtype(frontend.dtype), what, np.dtype(dtype)))
            if frontend.D != gmm.D:
                raise ValueError("the front-end emits %d features, the models take %d" % (frontend.D, gmm.D))
            if frontend.n_streams != int(n_streams):
                raise ValueError("the front-end has %d streams, the %s %d" % (frontend.n_streams, what, int(n_streams)))
        if endpointer is not None:
            if frontend is None:
                raise ValueError("an endpointer needs a front-end: online(..., frontend=StreamingFrontend(...), endpointer=...)")
            if endpointer.ctx is not ctx:
                raise ValueError("the endpointer lives on another context than the %s" % what)
            if endpointer.sample_rate != frontend.sample_rate:
                raise ValueError("the endpointer takes %d Hz, the front-end %d Hz" % (endpointer.sample_rate, frontend.sample_rate))
            if endpointer.n_streams != int(n_streams):
                raise ValueError("the endpointer has %d streams, the %s %d" % (endpointer.n_streams, what, int(n_streams)))
            if frontend.max_chunk < endpointer.max_piece:
                raise ValueError("the front-end takes chunks of %d samples, the gate can hand out %d ('start boundary' %d + carry %d + "
                                 "the endpointer's max_chunk %d)" % (frontend.max_chunk, endpointer.max_piece, endpointer.boundary,
                                                                    endpointer.carry_cap, endpointer.max_chunk))
            if -(-endpointer.min_utterance // frontend.step) < 2:
                raise ValueError("the shortest utterance of this endpoint config has %d samples: fewer than 2 frames of %d samples' stride"
                                 % (endpointer.min_utterance, frontend.step))
        self._ctx, self._dtype, self._gmm = ctx, dtype, gmm
        self.frontend = frontend
        self.endpointer = endpointer
        self.n_streams = int(n_streams)
        self._frames = np.zeros(self.n_streams, dtype=np.int64)       # what the session holds, for the checks of a push

    @property
    def frames(self):
        """Frames every stream has taken since its last reset: int64 [n_streams]."""
        return self._frames.copy()

    def _ids(self, ids, distinct=True):
        a = np.asarray(ids)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("ids must be a one-dimensional sequence of stream indices")
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.n_streams):
            raise ValueError("stream ids must lie in [0, %d)" % self.n_streams)
        if distinct and len(np.unique(a)) != len(a):
            raise ValueError("a stream is named twice in one push")
        return a

    def push(self, ids, chunks):
        """Stream ids[i] takes the frames chunks[i], a [t_i, D] array (t_i = 0: the stream sits this tick out)."""
        ids = self._ids(ids)
        if len(chunks) != len(ids):
            raise ValueError("%d chunks for %d ids" % (len(chunks), len(ids)))
        D = self._gmm.D
        chunks = [np.asarray(c) for c in chunks]
        for c in chunks:
            if c.ndim != 2 or c.shape[1] != D:
                raise ValueError("a chunk must be a [t, %d] array, not one of shape %r" % (D, c.shape))
        counts = np.array([len(c) for c in chunks], dtype=np.int64)
        self._room(ids, counts)
        if not counts.sum():
            return
        batch = _hip.Batch(self._ctx, chunks, dtype=self._dtype)
        try:
            batch.loglik(self._gmm, fetch=False)
            self.session.push(batch, ids)
            self._frames[ids] += counts
            self._ctx.sync()                              # (the batch's matrix is read until the sweep is done)
        finally:
            batch.close()

    def push_batch(self, ids, batch, first=None, count=None):
        """Stream ids[u] takes the columns [first[u], first[u] + count[u]) of utterance u of a resident `_hip.Batch`
        (e.g. from `features_from_signals`; first None: 0, count None: to the utterance's end).  A batch without
        likelihoods gets them here (once); one that holds a likelihood matrix is taken as it is, so that it can be fed
        piecewise.  The work is only enqueued: keep the batch alive until the context is synchronised (`result` does)."""
        ids = self._ids(ids)
        if batch.U != len(ids):
            raise ValueError("%d utterances for %d ids" % (batch.U, len(ids)))
        if batch.D != self._gmm.D:
            raise ValueError("the batch has %d feature dimensions, the model %d" % (batch.D, self._gmm.D))
        T = np.asarray(batch.lengths, dtype=np.int64)
        first = np.zeros(len(ids), dtype=np.int64) if first is None else np.asarray(first, dtype=np.int64)
        count = T - first if count is None else np.asarray(count, dtype=np.int64)
        if first.shape != T.shape or count.shape != T.shape or np.any(first < 0) or np.any(count < 0) or np.any(first + count > T):
            raise ValueError("first / count must name column ranges inside the batch's utterances")
        self._room(ids, count)
        if not count.sum():
            return
        if batch.S is None:
            batch.loglik(self._gmm, fetch=False)
        elif batch.S != self._gmm.S:
            raise ValueError("the batch holds likelihoods of %d states, the model has %d" % (batch.S, self._gmm.S))
        self.session.push(batch, ids, first, count)
        self._frames[ids] += count

    def push_audio(self, ids, chunks, end=None):
        """Stream ids[i] takes the int16 samples chunks[i] through the `StreamingFrontend` (`online(..., frontend=)`) and
        then the frames those samples made final; end[i] true ends the utterance's audio (its remaining frames come out;
        `finish` then frees the id).  The frames every stream will receive are computed on the host first: a push that the
        front-end would refuse, or one the streams have no room for, raises ValueError with nothing moved in either
        object."""
        if self.frontend is None:
            raise ValueError("this %s has no front-end: online(..., frontend=StreamingFrontend(...))" % self._what)
        ids, chunks, end, counts = self.frontend.plan(ids, chunks, end)
        self._room(ids, counts)
        batch = self.frontend._push(ids, chunks, end, counts)
        try:
            if counts.sum():
                self.push_batch(ids, batch)
                self._ctx.sync()                          # (the batch's matrix is read until the sweep is done)
        finally:
            batch.close()

    def _gated(self, ids, chunks, end):
        """The gate loop of `push_recording`: what the endpointer lets through goes on through `push_audio`; yields, per
        round of the gate, (the streams of the round, those whose utterance ended with it, their (begin, stop, open))."""
        if self.endpointer is None:
            raise ValueError("this %s has no endpointer: online(..., frontend=..., endpointer=StreamingEndpointer(...))" % self._what)
        for r_ids, pieces, flags, ranges in self.endpointer.gate(ids, chunks, end):
            try:
                self.push_audio(r_ids, pieces, flags)
            except ValueError as e:
                raise ValueError("streams %s: the %s refused what the endpointer let through (%s); the endpointer has moved: "
                                 "reset these streams" % (r_ids.tolist(), self._what, e))
            yield r_ids, r_ids[flags], [rg for rg in ranges if rg is not None]

    def reset(self, ids=None):
        """The streams `ids` (None: all) start again at frame 0 -- and, with an endpointer, at sample 0 of a new
        recording, where a front-end with running statistics (`RunningNorm`) starts them again at the prior."""
        ids = None if ids is None else self._ids(ids, distinct=False)
        if self.endpointer is not None:
            self.endpointer.reset(ids)
        self._reset_utterance(ids)
        if getattr(self.frontend, "reset_stats", None) is not None:
            self.frontend.reset_stats(ids)

    def _reset_utterance(self, ids):
        self.session.reset(ids)
        if self.frontend is not None:
            self.frontend.reset(ids)
        if ids is None:
            self._frames[:] = 0
        else:
            self._frames[ids] = 0

    def close(self):
        self.session.close()


class OnlineDecoder(_OnlineStreams):
    """Decode while the audio is still arriving: `n_streams` utterances take feature frames chunk by chunk, and
    `result` gives at any time what `ContinuousDecoder.decode_batch` would give for the frames pushed so far -- the same
    words, end costs, chosen ends and paths, without decoding the prefix again (the dynamic program of a stream is
    carried on the device: its previous column and its decision history, gh_online).

        dec = ContinuousDecoder(models, grammar="loop", word_penalty=p)
        on = dec.online(n_streams=64, max_frames=3000)
        on.push([3, 7], [frames_of_3, frames_of_7])          # [t_i, D] arrays, t_i >= 0
        words, info = on.result([3])                          # running hypothesis of stream 3
        words, info = on.finish([7])                          # ... of stream 7, whose id is free again

    `max_frames` is a hard capacity per stream.  Bad arguments (an id twice in one push or out of range, a chunk of
    another feature dimension, a push past `max_frames`) raise ValueError before the GPU is touched, and no stream moves.

    THE SETTLED PREFIX.  `commit` traces back from every cell of a stream's newest column that is still alive; where all
    those traces meet, everything before is final whatever audio follows.  It returns the words that became final with
    this call, `settled` all of them so far, and they are a prefix of every later `result`:

        on = dec.online(n_streams=64, window=400)             # history for 400 UNSETTLED frames per stream
        on.push(ids, chunks); new_words = on.commit(ids)      # per stream: words that can no longer change
        words, info = on.result([3])                          # settled words + the words of the unsettled tail

    With `window=` instead of `max_frames=` a stream may run for any length: the history is a ring that holds the frames
    behind the settled prefix, and a push that would take a stream's unsettled frames (frames - settled_frames) past the
    window raises ValueError like one past `max_frames`.  By default a commit forces nothing: a stream whose traces have
    not met within the window cannot take more frames and can only be finished (`max_tail=`, below, bounds the tail).  A
    windowed decoder offers no paths.

    THE FORCED COMMIT.  `online(..., max_tail=M)` (a decoder of up to 16 words, 1 <= M < window) bounds the unsettled tail:

        on = dec.online(n_streams=64, window=400, max_tail=300)
        on.push(ids, chunks); new_words = on.commit(ids)      # afterwards frames - settled_frames <= 300, always

    `commit` then runs the natural commit as ever; a stream that still holds more than M unsettled frames is FORCED
    (gh_online_force): the cell A in which the trace of its chosen end arrives in column frames - 1 - M is found, every
    live cell of the newest column whose trace does not pass A is removed (+inf), and a second commit settles up to A at
    least.  The words of both commits come back in order, in the usual shape.  The chosen end survives, so `result` gives
    the same words before and after, and the settled words stay a prefix of every later `result`; but from its first
    forced tick on a stream is the carried decode with those cells removed, no longer the one-shot decode of its prefix.
    `n_forced` counts per stream the commits that removed something (`reset` / `finish` clear it).  GUARANTEE: with a
    `commit` after every push of at most window - M frames, no push is ever refused for the window.

    AUDIO.  With a `sr.feature.StreamingFrontend` the streams take int16 PCM instead of feature frames:

        fe = StreamingFrontend(n_streams=64, normalize=feature_stats(training_signals))
        on = dec.online(n_streams=64, max_frames=3000, frontend=fe)
        on.push_audio([3, 7], [pcm_of_3, pcm_of_7])            # chunks of any length; the frames they make final are decoded
        on.push_audio([3], [last_piece], end=[True])            # the utterance's audio ends: its remaining frames come out
        words, info = on.finish([3])                            # ... and the id is free in both objects

    `reset` / `finish` reset the front-end's streams too; `push` / `push_batch` keep working beside `push_audio`.

    RECORDINGS.  A microphone stream carries no end flag.  With a `sr.audio_capture.StreamingEndpointer` as well, the
    streams take the recording as it arrives and the utterances are cut out by the endpoint detector:

        ep = StreamingEndpointer(n_streams=64, config=default_config(16000), max_chunk=3200)
        fe = StreamingFrontend(n_streams=64, normalize=stats, max_chunk=ep.max_piece)
        on = dec.online(n_streams=64, window=400, frontend=fe, endpointer=ep)
        for utt in on.push_recording([3, 7], [pcm_of_3, pcm_of_7]):       # every tick; end=[...] ends a recording
            print(utt["stream"], utt["words"], utt["begin"], utt["stop"], utt["open"])

    `push_recording` returns the utterances that ended with this call; `begin` / `stop` are the slice of the recording
    (`trim_ranges` of the offline detection; a recording without a segment yields no utterance).  The audio crosses the
    host link twice, once for the endpointer and once for the front-end.  If the decoder or the front-end refuses a
    piece (`max_frames`, `window`), the endpointer has already moved: `push_recording` raises ValueError naming the
    streams, and they must be `reset`.  With an endpointer `reset` starts a new RECORDING (all three objects), `finish`
    a new utterance (decoder and front-end only).

    WORD TIMES.  `online(..., times=True)` keeps the begin frame of every word beside the word (the column of the first
    cell of its run, `path_to_word_times`; an absolute frame index since the stream's last reset, also with `window=`
    after the ring has wrapped):

        on = dec.online(n_streams=64, window=400, times=True)
        new_words, new_begins = on.commit(ids, want_times=True)   # a settled word's begin is known at once ...
        words, info = on.result([3]); info["begins"][0]            # ... its end is the next word's begin (`word_spans`)

    `result` / `finish` add `info["begins"]`, `settled_times` gives the begins of all settled words, `push_recording`
    dicts gain `begins` (frames inside the utterance) and `word_begin` (recording samples: `begin` + frame x the
    front-end's `step`).  With times=False nothing changes and `want_times=True` raises ValueError.

    MORE THAN 16 WORDS.  A decoder of 17 to 64 words (2..8 states per word) runs on the wide session (gh_online_create_wide:
    one wave per stream, lane = word), with the same `push` / `push_batch` / `push_audio` / `push_recording` / `result` /
    `finish` / `reset` / `frames` and word times, and `result` is bitwise the one-shot decode of the frames pushed so far.
    Made like this it keeps the whole history (256 B per frame and stream) and NOTHING SETTLES: `online(..., window=)`
    raises `_hip.Unsupported` before the GPU is touched, and so do `commit`, `settled` and `settled_times`.  The settled
    prefix is opt-in (gh_online_create_wide_settle: the settle walk over 64 word lanes, a wave per stream):

        on = dec.online(n_streams=64, max_frames=3000, settle=True)       # full history (paths), with `commit`
        on = dec.online(n_streams=64, window=400, settle=True)            # history for 400 UNSETTLED frames per stream

    With `settle=True`, `commit`, `settled`, `settled_times`, the windowed `result` (no paths), the window check of a
    push and `push_recording`'s commit after every tick are the ones described above, unchanged; there is no forced
    commit either.  A decoder of up to 16 words always settles: `settle` changes nothing for it."""

    wide = False                                          # more than 16 words: the wide session
    settles = True                                        # ... which settles only where `settle=True` asked for it

    max_tail = None                                       # the bound of the forced commit (None: commits force nothing)

    def __init__(self, decoder, n_streams, max_frames=None, window=None, frontend=None, endpointer=None, times=False, settle=False,
                 max_tail=None):
        if decoder.grammar != "loop":
            raise _hip.Unsupported("online decoding takes the word-loop grammar (grammar='loop'), not %r%s"
                                   % (decoder.grammar, " (online_bigram takes it)" if decoder.grammar == "bigram" else
                                      " (online_layers takes it)" if decoder.grammar == "layers" else ""))
        if (max_frames is None) == (window is None):
            raise ValueError("exactly one of max_frames and window must be given")
        if int(n_streams) < 1 or int(window if max_frames is None else max_frames) < 1:
            raise ValueError("n_streams and max_frames / window must be positive")
        # more than 16 words: the wide session (a wave per stream), which keeps its full history and does not settle unless
        # settle=True asks for it
        self.wide = int(np.max(decoder.row_state)) // int(decoder.n) + 1 > 16
        self.settles = not self.wide or bool(settle)
        if max_tail is not None:
            if int(max_tail) < 1:
                raise ValueError("max_tail must be at least 1 (the newest column never settles), not %r" % (max_tail,))
            if window is not None and int(max_tail) >= int(window):
                raise ValueError("max_tail=%d must be smaller than window=%d: a push needs room" % (int(max_tail), int(window)))
            if self.wide:
                raise _hip.Unsupported("the forced commit (max_tail=) of a decoder with more than 16 words is not built yet")
            self.max_tail = int(max_tail)
        if not self.settles and window is not None:
            raise _hip.Unsupported("a decoder with more than 16 words keeps its full history: online(..., max_frames=), not window= "
                                   "(online(..., window=, settle=True) makes one that settles)")
        self._attach(decoder.ctx, decoder.dtype, decoder.gmm, n_streams, frontend, endpointer)
        self.decoder = decoder
        self.max_frames = None if max_frames is None else int(max_frames)
        self.window = None if window is None else int(window)
        if self.wide and not self.settles:
            self.session = _hip.OnlineWideSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames)
        elif self.wide and window is None:
            self.session = _hip.OnlineWideSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames, settle=True)
        elif self.wide:
            self.session = _hip.OnlineWideSession(decoder.ctx, decoder.lat, self.n_streams, window=self.window)
        elif window is None:
            self.session = _hip.OnlineSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames)
        else:
            self.session = _hip.OnlineSession(decoder.ctx, decoder.lat, self.n_streams, window=self.window)
        self._init_words(decoder, times)

    def _init_words(self, decoder, times):
        self._settled = np.zeros(self.n_streams, dtype=np.int64)      # settled frames (anchor column + 1) of every stream
        self._words = [[] for _ in range(self.n_streams)]             # ... and its settled words
        self.times = bool(times)
        self._begins = [[] for _ in range(self.n_streams)]            # times=True: the begin frames of the settled words
        self.n_forced = np.zeros(self.n_streams, dtype=np.int64)      # max_tail=: commits of a stream that pruned something
        self._row_word = np.where(decoder.row_state >= 0, decoder.row_state // decoder.n, -1).astype(np.int32)

    def _room(self, ids, counts):
        if self.window is not None:
            tail = self._frames[ids] + counts - self._settled[ids]
            if np.any(tail > self.window):
                k = int(np.flatnonzero(tail > self.window)[0])
                raise ValueError("stream %d would hold %d unsettled frames, window %d" % (ids[k], tail[k], self.window))
            return
        over = self._frames[ids] + counts > self.max_frames
        if np.any(over):
            k = int(np.flatnonzero(over)[0])
            raise ValueError("stream %d would hold %d frames, capacity %d" % (ids[k], self._frames[ids[k]] + counts[k], self.max_frames))

    def result(self, ids=None, want_path=False):
        """(word-index lists, dict(end_cost [n, n_end], best_end [n], frames [n][, paths])) of the streams `ids` (None:
        all) for the frames pushed so far: what `decode_batch` returns for those frames as whole utterances."""
        ids = np.arange(self.n_streams, dtype=np.int64) if ids is None else self._ids(ids, distinct=False)
        dec = self.decoder
        tm = dict(want_begin=True) if self.times else {}
        if self.window is not None:
            if want_path:
                raise ValueError("a decoder with a window offers no paths")
            r = self.session.tail(ids, row_label=self._row_word, max_labels=self._frames[ids] - self._settled[ids] + 2, **tm)
            if self.times:                                # the settled begins followed by the tail's
                r["begins"] = [np.asarray(self._begins[k] + [int(b) for b in bl], dtype=np.int32) for k, bl in zip(ids, r["begins"])]
            return [self._words[k] + [int(w) for w in l] for k, l in zip(ids, r.pop("labels"))], r
        if want_path:
            r = self.session.result(ids, want_path=True)
            if self.times:
                wt = [path_to_word_times(p, dec.row_state, dec.n) for p in r["paths"]]
                r["begins"] = [np.asarray(b, dtype=np.int32) for _, b in wt]
                return [w for w, _ in wt], r
            return [path_to_words(p, dec.row_state, dec.n) for p in r["paths"]], r
        r = self.session.result(ids, row_label=self._row_word, max_labels=dec._max_labels(self._frames[ids]), **tm)
        return [[int(w) for w in l] for l in r.pop("labels")], r

    def _refuse_wide(self):
        raise _hip.Unsupported("a decoder with more than 16 words has no settled prefix: it keeps its full history, and result() "
                               "gives the running hypothesis (online(..., settle=True) makes one that has)")

    def commit(self, ids=None, want_times=False):
        """Settles what can no longer change of the streams `ids` (None: all; distinct): the list of the words that became
        final with THIS call, per stream.  Nothing is settled while a stream has fewer than two frames or no live cell, or
        while its traces do not meet.  want_times=True (a decoder with times=True): (new_words, new_begins), the begin
        frame of every newly settled word beside it.  With `max_tail=` the streams that still hold more than that many
        unsettled frames are forced and committed again; what both commits settled comes back in order."""
        if not self.settles:
            self._refuse_wide()
        if want_times and not self.times:
            raise ValueError("this decoder keeps no word times: online(..., times=True)")
        ids = np.arange(self.n_streams, dtype=np.int64) if ids is None else self._ids(ids)
        new, new_begins = self._commit(ids)
        if self.max_tail is not None:
            over = np.flatnonzero(self._frames[ids] - self._settled[ids] > self.max_tail)
            if len(over):
                pruned = self.session.force(ids[over], self.max_tail)
                self.n_forced[ids[over]] += np.asarray(pruned) > 0
                more, more_begins = self._commit(ids[over])
                for k, i in enumerate(over):
                    new[i] = new[i] + more[k]
                    if self.times:
                        new_begins[i] = new_begins[i] + more_begins[k]
        if not self.times:
            return new
        return (new, new_begins) if want_times else new

    def _commit(self, ids):
        """One commit of the session: (new words, new begins -- None without times) per stream, book-keeping done."""
        tm = dict(want_begin=True) if self.times else {}
        # (room for a word per unsettled frame: with skip arcs a word can pass in fewer than n - 1 column steps)
        r = self.session.commit(ids, row_label=self._row_word, max_labels=self._frames[ids] - self._settled[ids] + 2, **tm)
        new = [[int(w) for w in l] for l in r["labels"]]
        for k, s, ws in zip(ids, r["settled_frames"], new):
            self._settled[k] = s
            self._words[k] = self._words[k] + ws
        if not self.times:
            return new, None
        new_begins = [[int(b) for b in bl] for bl in r["begins"]]
        for k, bs in zip(ids, new_begins):
            self._begins[k] = self._begins[k] + bs
        return new, new_begins

    def settled(self, ids=None):
        """(all settled words so far, settled_frames [n]) of the streams `ids` (None: all): stream k's first
        settled_frames[k] frames can no longer change its words."""
        if not self.settles:
            self._refuse_wide()
        ids = np.arange(self.n_streams, dtype=np.int64) if ids is None else self._ids(ids, distinct=False)
        return [list(self._words[k]) for k in ids], self._settled[ids].copy()

    def settled_times(self, ids=None):
        """The begin frames of all settled words so far of the streams `ids` (None: all), aligned with `settled`'s words
        (a decoder with times=True)."""
        if not self.settles:
            self._refuse_wide()
        if not self.times:
            raise ValueError("this decoder keeps no word times: online(..., times=True)")
        ids = np.arange(self.n_streams, dtype=np.int64) if ids is None else self._ids(ids, distinct=False)
        return [list(self._begins[k]) for k in ids]

    def push_recording(self, ids, chunks, end=None):
        """Stream ids[i] takes the int16 samples chunks[i] of its RECORDING through the decoder's `StreamingEndpointer`
        (`online(..., endpointer=)`); what its gate lets through goes on through `push_audio` (with `window=`, followed by
        `commit`), and utterances that ended are finished.  end[i] true ends the recording.  Returns the finished
        utterances in order: dicts `stream`, `words`, `begin`, `stop` (recording sample coordinates), `open` (the
        recording ended while speech was open).  A bad argument raises ValueError with nothing moved; a piece that the
        decoder or the front-end refuses raises ValueError AFTER the endpointer has moved: the streams it names must be
        `reset`.  A decoder with times=True adds `begins` (the frame inside the utterance every word begins in) and
        `word_begin` (the same in recording samples: `begin` + frame x the front-end's `step`)."""
        out = []
        for r_ids, done, ranges in self._gated(ids, chunks, end):
            if self.window is not None:
                self.commit(r_ids)
            if len(done):
                words, info = self.result(done)
                self._reset_utterance(done)
                for i, (k, w, rg) in enumerate(zip(done, words, ranges)):
                    utt = dict(stream=int(k), words=w, begin=int(rg[0]), stop=int(rg[1]), open=bool(rg[2]))
                    if self.times:
                        utt["begins"] = [int(b) for b in info["begins"][i]]
                        utt["word_begin"] = [int(rg[0]) + b * int(self.frontend.step) for b in utt["begins"]]
                    out.append(utt)
        return out

    def _reset_utterance(self, ids):
        super()._reset_utterance(ids)                     # ... and nothing is settled
        if ids is None:
            self._settled[:] = 0
            self.n_forced[:] = 0
        else:
            self._settled[ids] = 0
            self.n_forced[ids] = 0
        for k in (range(self.n_streams) if ids is None else ids):
            self._words[int(k)] = []
            self._begins[int(k)] = []

    def finish(self, ids, want_path=False):
        """`result(ids)` followed by a reset of the decoder's and the front-end's streams: the final decode of utterances
        that have ended; their ids are free (an endpointer's recording goes on)."""
        out = self.result(ids, want_path=want_path)
        self._reset_utterance(None if ids is None else self._ids(ids, distinct=False))
        return out


class OnlineBigramDecoder(OnlineDecoder):
    """`OnlineDecoder` for a decoder with a bigram grammar: the same streams, the same `push` / `push_batch` /
    `push_audio` / `push_recording` / `result` / `finish` / `reset` / `frames` and word times, over the carried bigram
    sweep (gh_online_create_bigram).  `result` gives at any time what `decode_batch` gives for the frames pushed so far.

        dec = ContinuousDecoder(models, grammar="bigram", bigram=BigramModel(...), lm_scale=8.0)
        on = dec.online_bigram(n_streams=64, max_frames=3000, times=True)
        on.push([3, 7], [frames_of_3, frames_of_7])
        words, info = on.result([3]); info["begins"][0]

    Made like this it has the surface of an `OnlineDecoder` made with `max_frames=`: the whole history is kept,
    `max_frames` is a hard capacity, and NOTHING SETTLES -- `commit`, `settled` and `settled_times` raise
    `_hip.Unsupported`.  The settled prefix is opt-in (gh_online_create_bigram_settle: the settle walk over the bigram
    records, where a first state is left through the predecessor word its own record names):

        on = dec.online_bigram(n_streams=64, window=400, times=True)      # history for 400 UNSETTLED frames per stream
        on.push(ids, chunks); new_words, new_begins = on.commit(ids, want_times=True)
        words, info = on.result([3])                                      # settled words + the words of the unsettled tail
        on = dec.online_bigram(n_streams=64, max_frames=3000, settle=True)   # full history (paths), with `commit`

    With `window=`, or with `max_frames=..., settle=True`, `commit`, `settled`, `settled_times`, the windowed `result`
    (no paths), the window check of a push and `push_recording`'s commit after every tick are `OnlineDecoder`'s own,
    unchanged; there is no forced commit either.

    MORE THAN 16 WORDS.  `online_bigram(..., wide=True)` lets a decoder of 17 to 64 words (2..8 states per word) run on the
    wide bigram session (gh_online_create_bigram_wide: one wave per stream, lane = word, the word-to-word costs in LDS):

        on = dec.online_bigram(n_streams=64, max_frames=3000, times=True, wide=True)

    with the same `push` / `push_batch` / `push_audio` / `push_recording` / `result` / `finish` / `reset` / `frames` and
    word times, and `result` is bitwise the one-shot decode of the frames pushed so far.  It keeps the whole history (256 B
    per frame and stream) and nothing settles: `wide=True` with `window=` or `settle=True` raises `_hip.Unsupported` before
    the GPU is touched (under wide=True the settled prefix is not built yet: wide="settle" has it), and `commit`, `settled`
    and `settled_times` are refused.  `wide=True` is a permission, not a demand: a decoder of up to 16 words is served
    exactly as without it.  Without it a decoder of more than 16 words is refused by the library, as before.

    THE SETTLED PREFIX BEYOND 16 WORDS is asked for by name (gh_online_create_bigram_wide_settle: the settle walk over 64
    word lanes, a wave per stream, where a first state is left through the predecessor word its own record names):

        on = dec.online_bigram(n_streams=64, window=400, times=True, wide="settle")         # 400 UNSETTLED frames per stream
        on = dec.online_bigram(n_streams=64, max_frames=3000, settle=True, wide="settle")   # full history (paths), with `commit`
        on = dec.online_bigram(n_streams=64, max_frames=3000, wide="settle")                # as wide=True: nothing settles

    `wide="settle"` is a permission like `wide=True`: up to 16 words it changes nothing, beyond 16 words `window=` and
    `settle=True` mean what they mean for a narrow bigram decoder -- `commit`, `settled`, `settled_times`, the windowed
    `result` (no paths), the window check of a push and `push_recording`'s commit after every tick, unchanged; device memory
    per stream is then (window + 1) x 256 B + the 512 n B column instead of max_frames x 256 B.  There is no forced commit,
    and words of 12 or 16 states are not offered beyond 16 words.  Any other value of `wide` is a ValueError."""

    def __init__(self, decoder, n_streams, max_frames=None, window=None, frontend=None, endpointer=None, times=False, settle=False,
                 wide=False):
        if decoder.grammar != "bigram":
            raise _hip.Unsupported("online_bigram takes the bigram grammar (grammar='bigram'), not %r%s"
                                   % (decoder.grammar, " (online takes it)" if decoder.grammar == "loop" else
                                      " (online_layers takes it)" if decoder.grammar == "layers" else ""))
        if (max_frames is None) == (window is None):
            raise ValueError("exactly one of max_frames and window must be given")
        if int(n_streams) < 1 or int(window if max_frames is None else max_frames) < 1:
            raise ValueError("n_streams and max_frames / window must be positive")
        if not (isinstance(wide, (bool, np.bool_)) or (isinstance(wide, str) and wide == "settle")):
            raise ValueError("wide must be False, True or 'settle', not %r" % (wide,))
        # more than 16 words, and the caller allows it: the wide bigram session (a wave per stream); it settles, and may have
        # a window, only where wide="settle" asked for that by name
        self.wide = bool(wide) and int(np.max(decoder.row_state)) // int(decoder.n) + 1 > 16
        if self.wide and not isinstance(wide, str) and (window is not None or settle):
            raise _hip.Unsupported("under wide=True the settled prefix of a wide bigram session (more than 16 words) is not built yet: "
                                   "online_bigram(..., max_frames=, wide=True) without window= and settle=True, or "
                                   "online_bigram(..., wide=\"settle\") with them")
        self._attach(decoder.ctx, decoder.dtype, decoder.gmm, n_streams, frontend, endpointer)
        self.decoder = decoder
        self.max_frames = None if max_frames is None else int(max_frames)
        self.window = None if window is None else int(window)
        self.settles = bool(settle) or window is not None
        # a ONE-WORD bigram grammar is a word loop -- one entry row, fed by the word's own last state -- and the library
        # recognises its graph in the loop form: the loop session serves it, with the same rows and the same results
        if int(decoder.lat.n_end[0]) == 1 and "bigram" not in decoder.lat.forms():
            self.session = _hip.OnlineSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames, self.window)
        elif self.wide and not self.settles:
            self.session = _hip.OnlineBigramWideSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames)
        elif self.wide and window is None:
            self.session = _hip.OnlineBigramWideSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames, settle=True)
        elif self.wide:
            self.session = _hip.OnlineBigramWideSession(decoder.ctx, decoder.lat, self.n_streams, window=self.window)
        elif not self.settles:
            self.session = _hip.OnlineBigramSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames)
        elif window is None:
            self.session = _hip.OnlineBigramSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames, settle=True)
        else:
            self.session = _hip.OnlineBigramSession(decoder.ctx, decoder.lat, self.n_streams, window=self.window)
        self._init_words(decoder, times)                              # (a decoder that does not settle: the settled words stay empty)

    def _refuse(self):
        raise _hip.Unsupported("this bigram decoder has no settled prefix: result() gives the running hypothesis "
                               "(online_bigram(..., window=) or (..., max_frames=, settle=True) makes one that has)")

    def commit(self, ids=None, want_times=False):
        if not self.settles:
            self._refuse()
        return super().commit(ids, want_times)

    def settled(self, ids=None):
        if not self.settles:
            self._refuse()
        return super().settled(ids)

    def settled_times(self, ids=None):
        if not self.settles:
            self._refuse()
        return super().settled_times(ids)


class OnlineLayersDecoder(OnlineDecoder):
    """`OnlineDecoder` for a decoder with the K-layer lattice, the reference's own continuous recogniser (main.py:35): the
    same streams, the same `push` / `push_batch` / `push_audio` / `push_recording` / `result` / `finish` / `reset` /
    `frames` and word times, over the carried layer sweep (gh_online_create_layers: one wave per stream, lane = (layer
    mod 4, word)).

        dec = ContinuousDecoder(models, n_layers=7)
        on = dec.online_layers(n_streams=64, max_frames=1000, times=True)
        on.push([3, 7], [frames_of_3, frames_of_7])
        words, info = on.result([3]); info["begins"][0]

    From two frames on `result` gives what `decode_batch` gives for the frames pushed so far: exactly `n_layers` words
    once the frames hold that many, no words (and +inf end costs) before.  A stream that holds exactly ONE frame reports
    the causal column 0: its end costs, the chosen end among them, no words and an empty path (`decode_batch` of a
    one-frame utterance takes the reference's column wrap instead, which on a layer lattice reads the column being
    filled; a stream cannot know that it will stay at one frame).

    An utterance of exactly K words is bounded in length, so the whole history is kept, `max_frames` is a hard capacity
    (128 B per frame and stream at 5 states without skip arcs) and NOTHING SETTLES: there is no `window=`, and `commit`,
    `settled` and `settled_times` raise `_hip.Unsupported`.  Taken: 1 to 8 layers of up to 16 words of 2 to 8 states.  Not
    offered yet, refused by the library by name: 9 to 16 layers, words of 12 or 16 states, 17 to 64 words per layer."""

    settles = False

    def __init__(self, decoder, n_streams, max_frames, frontend=None, endpointer=None, times=False):
        if decoder.grammar != "layers":
            raise _hip.Unsupported("online_layers takes the K-layer lattice (grammar='layers'), not %r%s"
                                   % (decoder.grammar, " (online takes it)" if decoder.grammar == "loop" else
                                      " (online_bigram takes it)" if decoder.grammar == "bigram" else ""))
        if max_frames is None or int(n_streams) < 1 or int(max_frames) < 1:
            raise ValueError("n_streams and max_frames must be positive")
        self._attach(decoder.ctx, decoder.dtype, decoder.gmm, n_streams, frontend, endpointer)
        self.decoder = decoder
        self.max_frames, self.window = int(max_frames), None
        self.session = _hip.OnlineLayersSession(decoder.ctx, decoder.lat, self.n_streams, self.max_frames)
        self._init_words(decoder, times)                              # (nothing settles: the settled words stay empty)

    def _refuse(self):
        raise _hip.Unsupported("a decoder on the K-layer lattice has no settled prefix: it keeps its full history, and result() gives "
                               "the running hypothesis")

    def commit(self, ids=None, want_times=False):
        self._refuse()

    def settled(self, ids=None):
        self._refuse()

    def settled_times(self, ids=None):
        self._refuse()


class OnlineWordRecognizer(_OnlineStreams):
    """Isolated-word recognition while the audio is still arriving: `n_streams` utterances take feature frames chunk by
    chunk, and `result` gives at any time what `IsolatedWordRecognizer.recognize` would give for the frames pushed so far,
    without scoring the prefix again.  The reference's `record` action (cli.py:44-66: record, detect_endpoints, MFCC,
    `m.evaluate(x)` for every word model, arg-min) as a live path:

        rec = IsolatedWordRecognizer(models)
        on = rec.online(n_streams=64)
        on.push([3, 7], [frames_of_3, frames_of_7])          # [t_i, D] arrays, t_i >= 0
        words, info = on.result([3])                          # running arg-min word of stream 3; info["costs"] [n, W]
        words, info = on.finish([7])                          # ... of stream 7, whose id is free again

    THE CONTRACT.  For a stream that holds k >= 2 frames, `result` is what `IsolatedWordRecognizer` gives for those k
    frames as a whole utterance: on the same likelihood matrix the costs are bitwise equal, and the word is their
    np.argmin (the first of equal minima, core.py:82-87).  For a stream that holds exactly ONE frame, `result` gives
    column 0 of every longer decode: a word's cost is its first state's emission if that state is also its last, +inf
    otherwise.  The reference's one-frame special case is NOT reproduced: it is the column wrap of decode.py:109-114,
    which lets row r read row r-1 of the same column.  Utterances cut by an endpointer always have >= 2 frames.  A stream
    without frames gives +inf costs and word -1.

    A word chain needs no decision history to report its cost, so a stream is ONE cost column on the device (W x n
    doubles: 400 B at 10 words x 5 states).  Streams may run for any length: there is no capacity argument, no window and
    nothing to settle.  Bad arguments (an id twice in one push or out of range, a chunk of another feature dimension, a
    column range outside its utterance) raise ValueError before the GPU is touched, and no stream moves.

    MODELS.  Mixture recognisers -- one-component mixtures included -- run `batch.loglik` and the carried sweep.  A
    recogniser of single-Gaussian word models (use_gmm=False: scored by mahalanobis inside the fused kernel, which has no
    carried form) raises `_hip.Unsupported`.

    AUDIO and RECORDINGS work as in `OnlineDecoder`: with `frontend=` the streams take int16 PCM (`push_audio`), with
    `endpointer=` as well whole recordings, and `push_recording` returns the utterances that ended with the call as dicts
    `stream`, `word`, `costs` [W], `begin`, `stop` (recording sample coordinates) and `open`.  With an endpointer `reset`
    starts a new RECORDING (all three objects), `finish` a new utterance (recogniser and front-end only).

    CONFIDENCE.  `online(..., soft=True, scale=, log_prior=)`: every stream carries one more column, the log-alphas of the
    forward sweep, and `result` / `finish` add `soft_costs`, `posteriors`, `confidence` and `soft_words` to their info dict
    (as `recognize(want_posteriors=True)`; `push_recording` dicts gain `confidence`).  From ONE frame on the soft costs are
    bitwise `soft_costs` of the frames so far on the same likelihoods, and the posteriors come from the same
    `vocabulary_posteriors`.  A stream without frames: soft costs +inf, a row of zeros, confidence 0.0."""

    _what = "recogniser"

    def __init__(self, recognizer, n_streams, frontend=None, endpointer=None, soft=False, scale=1.0, log_prior=None):
        if recognizer.single:
            raise _hip.Unsupported("online word recognition takes mixture word models: single-Gaussian models (use_gmm=False) are "
                                   "scored inside the fused sweep, which has no carried form")
        if int(n_streams) < 1:
            raise ValueError("n_streams must be positive")
        self.soft = bool(soft)
        if self.soft:
            self._scale, self._log_prior = _posterior_args(recognizer.W, scale, log_prior)
        self._attach(recognizer.ctx, recognizer.dtype, recognizer.gmm, n_streams, frontend, endpointer)
        self.recognizer = recognizer
        self.session = _hip.WordStreamSession(recognizer.ctx, recognizer.lat, self.n_streams, **({"soft": True} if self.soft else {}))

    def _room(self, ids, counts):
        pass                                              # (a stream holds one column: it takes any number of frames)

    def result(self, ids=None):
        """(words int64 [n], dict(costs [n, W], frames [n])) of the streams `ids` (None: all) for the frames pushed so far:
        what `recognize` returns for those frames as whole utterances (a stream without frames: word -1, costs +inf).
        A soft recogniser adds soft_costs, posteriors, confidence and soft_words."""
        ids = np.arange(self.n_streams, dtype=np.int64) if ids is None else self._ids(ids, distinct=False)
        r = self.session.result(ids)
        words, info = np.asarray(r["best"], dtype=np.int64), dict(costs=r["costs"], frames=r["frames"])
        if self.soft:                                     # soft_costs, posteriors, confidence, soft_words: as `recognize`
            info.update(_posterior_info(self.session.result_soft(ids), words, self._scale, self._log_prior))
        return words, info

    def push_recording(self, ids, chunks, end=None):
        """Stream ids[i] takes the int16 samples chunks[i] of its RECORDING through the recogniser's `StreamingEndpointer`
        (`online(..., endpointer=)`); what its gate lets through goes on through `push_audio`, and utterances that ended
        are finished.  end[i] true ends the recording.  Returns the finished utterances in order: dicts `stream`, `word`,
        `costs`, `begin`, `stop`, `open` (the recording ended while speech was open).  A bad argument raises ValueError with
        nothing moved; a piece that the front-end refuses raises ValueError AFTER the endpointer has moved: the streams it
        names must be `reset`."""
        out = []
        for _, done, ranges in self._gated(ids, chunks, end):
            if len(done):
                words, info = self.result(done)
                self._reset_utterance(done)
                for i, (k, w, c, rg) in enumerate(zip(done, words, info["costs"], ranges)):
                    out.append(dict(stream=int(k), word=int(w), costs=c, begin=int(rg[0]), stop=int(rg[1]), open=bool(rg[2])))
                    if self.soft:
                        out[-1]["confidence"] = float(info["confidence"][i])
        return out

    def finish(self, ids):
        """`result(ids)` followed by a reset of the recogniser's and the front-end's streams: the final scores of
        utterances that have ended; their ids are free (an endpointer's recording goes on)."""
        out = self.result(ids)
        self._reset_utterance(None if ids is None else self._ids(ids, distinct=False))
        return out


class InFlight:
    """Several batches in flight on ONE GPU: `n_lanes` contexts (HIP stream, scratch, pinned buffers), one host
    thread each, every lane with its own resident copy of whatever `make_worker(ctx)` builds (e.g. a recogniser).
    The host side of a batch (result copy-back, arg-min, Python) then overlaps the other lanes' kernels -- what
    `bench.py --inflight 2` measures (+17 % throughput on configs[1]).  ctypes releases the GIL during calls.

        pool = InFlight(lambda ctx: IsolatedWordRecognizer(models, ctx=ctx))
        results = pool.map(lambda rec, xs: rec.recognize(xs), list_of_utterance_lists)      # in input order
    """

    def __init__(self, make_worker, n_lanes=2, device=None):
        dev = _hip.default_context(device).device
        self.ctxs = [_hip.Context(dev) for _ in range(max(1, int(n_lanes)))]
        self.workers = [make_worker(c) for c in self.ctxs]

    def map(self, fn, items):
        import threading
        items = list(items)
        out = [None] * len(items)
        lock, state = threading.Lock(), {"next": 0, "err": None}

        def run(worker):
            try:
                while True:
                    with lock:
                        k = state["next"]
                        if k >= len(items) or state["err"] is not None:
                            return
                        state["next"] = k + 1
                    out[k] = fn(worker, items[k])
            except BaseException as e:  # surfaced in the caller's thread
                state["err"] = e
        threads = [threading.Thread(target=run, args=(w,)) for w in self.workers]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if state["err"] is not None:
            raise state["err"]
        return out

    def close(self):
        for w in self.workers:
            h = getattr(w, "lat", None)
            if h is not None and hasattr(h, "close"):
                h.close()
        for c in self.ctxs:
            _pack._gmm_cache.purge(c)     # handles are bound to the context they were created with
            _pack._lat_cache.purge(c)
            _pack._normal_cache.purge(c)
            c.close()
