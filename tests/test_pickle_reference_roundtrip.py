# -*- coding: utf-8 -*-
"""N2: model wire formats, checked against the REFERENCE's own pickle.

The reference persists models with pickle; this package keeps its module paths / class names / attribute names,
so (a) the reference's pickles load here (golden G12, also tested on the GPU tier) and (b) pickles EMITTED here
load in the reference and score identically there.  The reference's classes define no pickling hooks (no
__reduce__ / __getstate__ / __setstate__): what it builds from a pickle is fixed by the class names and the
attribute dicts the pickle carries.  (b) is therefore checked without the reference: both pickles are decoded with
stand-ins for the `sr` classes, and the emitted one must give the same object graph -- class names, attribute
names, arrays bit for bit, shared arrays shared -- as the reference's own pickle in G12, whose scores the
reference recorded there.  No GPU is needed: unpickling / pickling only moves parameters."""
import io
import pickle

import numpy as np

from conftest import load_golden


class _Stand:
    """Stand-in for an instance of one of the reference's `sr` classes: its class name and the state pickle gives it."""

    def __init__(self, name):
        self.name, self.state = name, None

    def __setstate__(self, state):
        self.state = state


def _decode(blob):
    """Unpickle with every `sr.*` class replaced by a _Stand (numpy and the standard library load as usual)."""
    classes = {}

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            if module != "sr" and not module.startswith("sr."):
                return super().find_class(module, name)
            key = module + "." + name
            if key not in classes:
                classes[key] = type(name, (), {"__new__": lambda cls, *a, _key=key: _Stand(_key)})
            return classes[key]
    return Unpickler(io.BytesIO(blob)).load()


def _graph(x, seen):
    """A comparable form of a decoded object graph; objects seen before (aliasing) become back-references."""
    if id(x) in seen:
        return ("ref", seen[id(x)])
    if isinstance(x, (_Stand, np.ndarray, list, dict)):
        seen[id(x)] = len(seen)
    if isinstance(x, _Stand):
        return ("obj", x.name, _graph(x.state, seen))
    if isinstance(x, np.ndarray):
        return ("array", x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, dict):
        return ("dict", tuple((k, _graph(v, seen)) for k, v in sorted(x.items())))
    if isinstance(x, (list, tuple)):
        return (type(x).__name__, tuple(_graph(v, seen) for v in x))
    if isinstance(x, float):
        return ("float", np.float64(x).tobytes())
    return (type(x).__name__, x)


def test_pickles_emitted_here_load_and_score_in_the_reference():
    g = load_golden("G12_reference_pickle")
    ref_blob = g["pickle"].tobytes()
    hmms = pickle.loads(ref_blob)                         # reference pickle -> mirror classes
    import sr.recognition.hmm as mirror_hmm
    assert type(hmms[0]) is mirror_hmm.HMM
    blob = pickle.dumps(hmms, protocol=2)                 # mirror classes -> pickle, as continuous_train writes them
    ref, emitted = _decode(ref_blob), _decode(blob)
    assert [h.name for h in emitted] == ["sr.recognition.hmm.HMM"] * len(g["evaluate"])
    assert _graph(emitted, {}) == _graph(ref, {})         # what the reference builds from it: the models it scored
    # the comparison sees a change in the last bit of one parameter
    hmms[-1].gmm_states[-1].dists[0].mean[0] = np.nextafter(hmms[-1].gmm_states[-1].dists[0].mean[0], np.inf)
    assert _graph(_decode(pickle.dumps(hmms, protocol=2)), {}) != _graph(ref, {})


def test_npz_model_format_round_trip(tmp_path):
    from sr.recognition.model_io import save_models_npz, load_models_npz, save_models_pickle, load_models_pickle
    g = load_golden("G12_reference_pickle")
    hmms = pickle.loads(g["pickle"].tobytes())
    p = str(tmp_path / "vocab.npz")
    save_models_npz(p, hmms)
    back = load_models_npz(p)
    assert len(back) == len(hmms)
    for a, b in zip(hmms, back):
        np.testing.assert_array_equal(a.transitions, b.transitions)
        for ga, gb in zip(a.gmm_states, b.gmm_states):
            np.testing.assert_array_equal(ga.w, gb.w)
            for da, db in zip(ga.dists, gb.dists):
                np.testing.assert_array_equal(da.mean, db.mean)
                np.testing.assert_array_equal(da.cov, db.cov)
    pp = str(tmp_path / "vocab.pkl")
    save_models_pickle(pp, back)
    again = load_models_pickle(pp)
    assert all(not (a != b) for x, y in zip(back, again) for a, b in zip(x.gmm_states, y.gmm_states))
