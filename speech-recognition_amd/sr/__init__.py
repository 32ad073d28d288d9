# -*- coding: utf-8 -*-
"""MI355X-native drop-in for the `sr` package's recognition core.

Provided: `sr.recognition` (the GMM-HMM hot path), `sr.feature` (the MFCC front-end),
`sr.langmodel` (lexical-tree spell check) and `sr.audio_capture` (the recorder's endpoint
detection, batched on the GPU; the live microphone loop is not mirrored).  The last two are
imported on their own, `import sr.langmodel`, `import sr.audio_capture`; the reference's
wav-file drivers (sr/core.py) are out of scope.  The names the reference re-exports from
`sr` (sr/__init__.py:2) are re-exported here too.
"""
from .core import delta_feature  # noqa: F401  (reference sr/__init__.py:1; the wav / file drivers are out of scope)
from .recognition import HMMState, HMM, decode_hmm_states, GMM, build_state_sequences, NES  # noqa: F401
