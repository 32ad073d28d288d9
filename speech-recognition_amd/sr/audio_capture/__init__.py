# -*- coding: utf-8 -*-
"""`sr.audio_capture` -- the reference's recorder (sr/audio_capture/record.py) with its endpoint detection on the GPU,
for whole batches of recordings (`detect_endpoints`) and for recordings that are still arriving (`StreamingEndpointer`).
Imports without `pyaudio`; only the live microphone loop needs it."""
from .record import *  # noqa: F401,F403
from .stream import StreamingEndpointer  # noqa: F401
