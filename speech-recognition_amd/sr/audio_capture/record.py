# -*- coding: utf-8 -*-
"""Mirror of sr/audio_capture/record.py.  The reference detects the speech in a recording inside a PyAudio callback,
one recording at a time, as a Python loop over frames (`record_callback`, :116-174; `classify_frame`, :176-217).  Here
that algorithm runs on the GPU for any number of recordings at once (`detect_endpoints`: csrc/gh_endpoint.hip), and
`AudioRecorder.process` puts one recording through the same path in place of the callback.  The microphone loop itself
is not mirrored: `start_recording` / `record` need `pyaudio`, which is imported lazily."""
import math
import os.path
import wave

import numpy as np

from ..recognition import _hip

__all__ = ["decode_audio_stream", "AudioFrame", "AudioRecorder", "record", "default_config", "derive_config",
           "detect_endpoints", "trim_ranges"]

PA_INT16 = 8                     # pyaudio.paInt16
PA_SAMPLE_WIDTH = 2              # PyAudio.get_sample_size(paInt16)
MAX_FRAME_UNITS = 1280           # csrc/gh_endpoint.hip: units of one frame that fit a wave's share of LDS


def decode_audio_stream(data, dtype=np.int16):
    return np.frombuffer(data, dtype).tolist()


class AudioFrame:
    def __init__(self, data, is_speech=False):
        self.data = data
        self.is_speech = is_speech
        # energy of the signal
        self.energy = 0
        # signal level
        self.level = 0

    def calc_energy(self):
        """record.py:23-31, on the host: it is one frame."""
        self.data = np.asarray(self.data)
        total = np.sum(self.data.astype(np.int64) ** 2)
        if total <= 1:
            self.energy = 0
        else:
            self.energy = 10 * np.log10(total)
        return self.energy


def default_config(sample_rate=8000):
    """The dict AudioRecorder() builds for config=None (record.py:58-74), at `sample_rate`."""
    return {
        'sample rate': sample_rate,
        'format': PA_INT16,
        'chunk size': 1024,
        'channel count': 1,
        'forget factor': 1,
        'max record time': 1000,
        'frame time': 0.02,  # in seconds
        'frame stride': 0.01,  # in seconds
        'adjustment': 0.01,
        'onset threshold': 3,
        'offset threshold': 0.2,
        'silence threshold': 500,  # in ms
        'speech threshold': 250,  # in ms
        'start boundary': 200,  # in ms
        'end boundary': 0,  # in ms
    }


def derive_config(config):
    """record.py:78-91 IN PLACE, like AudioRecorder.__init__: 'samples per frame' and 'frame stride' in samples, the two
    thresholds in frames, the two boundaries in samples.  A missing key is a KeyError, as in the reference."""
    config['samples per frame'] = int(config['frame time'] * config['sample rate'])
    config['frame stride'] = int(config['frame stride'] * config['sample rate'])
    if config['frame stride'] < 1:
        raise ValueError("'frame stride' is %d samples (must be >= 1)" % config['frame stride'])
    config['silence threshold'] = int(config['silence threshold'] * config['sample rate'] / (1000 * config['frame stride']))
    config['speech threshold'] = int(config['speech threshold'] * config['sample rate'] / (1000 * config['frame stride']))
    config['start boundary'] = int(config['start boundary'] / 1000 * config['sample rate'])
    config['end boundary'] = int(config['end boundary'] / 1000 * config['sample rate'])
    return config


_CLASSIFIER_KEYS = ('forget factor', 'adjustment', 'onset threshold', 'offset threshold')


def _derived(config, sample_rate=8000):
    """A derived config for the kernels, checked: None -> the default config; a dict that already has 'samples per frame'
    (an AudioRecorder's config) is taken as derived; any other dict is derived on a COPY (the caller's stays as it is)."""
    if config is None:
        config = default_config(sample_rate)
    if 'samples per frame' not in config:
        config = derive_config(dict(config))
    for k in _CLASSIFIER_KEYS + ('frame stride', 'silence threshold', 'speech threshold', 'start boundary'):
        if k not in config:
            raise KeyError(k)
    width, stride = config['samples per frame'], config['frame stride']
    if width < 1 or stride < 1 or stride > width:
        raise ValueError("frames of %d samples every %d: need 1 <= stride <= width" % (width, stride))
    g = math.gcd(int(width), int(stride))
    q = 8 if g % 8 == 0 else 4 if g % 4 == 0 else 2 if g % 2 == 0 else 1
    if width // q > MAX_FRAME_UNITS:
        raise ValueError("frames of %d samples every %d are %d units of %d samples; the energy kernel holds at most %d "
                         "(see detect_endpoints)" % (width, stride, width // q, q, MAX_FRAME_UNITS))
    return config


def _check_signals(signals):
    out = []
    for i, x in enumerate(signals):
        x = np.asarray(x)
        if x.dtype != np.int16:
            raise TypeError("recording %d has dtype %s: endpoint detection reads int16 samples" % (i, x.dtype))
        if x.ndim != 1:
            raise ValueError("recording %d has shape %s: one channel, 1-D" % (i, x.shape))
        out.append(x)
    return out


def detect_endpoints(signals, config=None, max_segments=1, want_frames=False, device=None):
    """Endpoint detection of `record_callback` for a list of 1-D int16 recordings, on the GPU.

    config: an AudioRecorder config as the user writes it (None: the reference's default, 8 kHz; it is derived on a copy),
    or an already derived one (`AudioRecorder.config`).  Returns a dict of arrays:
      start, end   [U, max_segments] int64: the reference's speech_start_index / speech_end_index per segment, 0 where
                   there is no segment
      n_segments   [U]; an open segment counts
      open         [U] bool: speech started and never ended; that segment's `end` is len(signal) - 1
      frames_done  [U]: frames the classifier went through (the one at which it stopped included)
    and with want_frames the ragged per-frame `is_speech` attribute, `level`, `background`, `energy` (lists of arrays,
    zero behind the frame at which detection stopped) and their `frame_off`.
    max_segments = 1 is the reference.  With more, detection re-arms after an end -- the segment is recorded, every piece
    of state (level, background, carried decision, both counters) stays as it is -- and stops at the cap.
    Recordings shorter than one chunk, or too short to reach frame 10, are valid and have no segment.
    Limit: the energy kernel sums a frame from units of Q samples, Q = the widest of 8, 4, 2, 1 that divides
    gcd(width, stride), and width / Q may not exceed 1280 -- 10 240 samples per frame when the gcd is a multiple of 8,
    1 280 when it is odd (44.1 kHz with 'frame time' 0.03 is 1323 / 441 samples: refused with a ValueError, here, before
    the GPU is touched).  Framings whose 64-frame tiles do not fit LDS run with shorter tiles; with an odd gcd and
    stride + width > 1280 that is one frame per wave, correct and slow."""
    cfg = _derived(config)
    if int(max_segments) < 1:
        raise ValueError("max_segments = %r" % (max_segments,))
    sigs = _check_signals(signals)
    return _hip.endpoints(_hip.default_context(device), sigs, cfg, int(max_segments), bool(want_frames))


def trim_ranges(result, lengths, config=None):
    """(begin, stop) of every utterance a result of `detect_endpoints` cuts out of recordings of `lengths` samples, in
    recording order: per segment the slice of get_samples (record.py:243-248), [max(start - 'start boundary', 0), end + 1)
    clipped to the recording; an open segment runs to the end of the recording.  A recording without any segment keeps
    its whole length (a deviation: the reference would return samples[0:1])."""
    begin, stop, _ = _hip.trim_ranges(result, lengths, _derived(config)['start boundary'])
    return begin, stop


class AudioRecorder:
    def __init__(self, config=None):
        """
        :param config: dictionary containing configuration of the AudioRecorder, with the reference's keys
                ('sample rate', 'format', 'chunk size', 'channel count', 'forget factor', 'max record time',
                'frame time', 'frame stride', 'adjustment', 'onset threshold', 'offset threshold',
                'silence threshold', 'speech threshold', 'start boundary', 'end boundary'); like the reference the
                derived values are written back into the dict that was given.
        """
        if config is None:
            config = default_config()
        self.config = derive_config(config)
        self.frames = []
        self.samples = []
        self.audio_driver = None      # a pyaudio.PyAudio, made by start_recording
        self.started_speech = False
        self.cache_data = {
            'background': 0, 'silence time': 0, 'speech time': 0, 'frame count': 0,
            'boundary sample count': 0
        }
        self.curr_delay = 0
        self.speech_start_index = 0
        self.speech_end_index = 0
        self.should_end_recording = False
        # debug information
        self.levels = []
        self.backgrounds = []
        self.final_levels = []

    def process(self, samples, device=None):
        """One int16 recording through the device path (a batch of one) in place of the PyAudio callback: fills
        `samples`, `speech_start_index`, `speech_end_index`, `started_speech` and the debug lists `levels`,
        `backgrounds`, `final_levels`, as long as the reference leaves them (frames 10 .. the frame at which it stopped).
        `samples` holds what the callback would have been handed in whole chunks of 'samples per frame': everything when
        speech never ended, else up to the chunk of the frame at which detection stopped plus the chunks the reference
        still appends while it waits for 'end boundary' samples (at least one: record.py:122-130).  The attributes are the
        reference's, quirks included: `speech_end_index` stays 0 when speech never ends.  The list of AudioFrame objects
        (`frames`) is NOT filled: the frames live on the device.  Returns self."""
        x = _check_signals([samples])[0]
        cfg = _derived(self.config)
        r = _hip.endpoints(_hip.default_context(device), [x], cfg, 1, True)
        width = cfg['samples per frame']
        done = int(r["frames_done"][0])
        has, is_open = int(r["n_segments"][0]) > 0, bool(r["open"][0])
        chunks = len(x) // width
        if has and not is_open:
            # frame i >= 1 arrives with chunk 1 + (i - 1) // int(width / stride); then one chunk per callback until
            # 'boundary sample count' >= 'end boundary', the first of them included (record.py:122-130)
            last = 1 + (done - 2) // int(width / cfg['frame stride'])
            chunks = min(chunks, last + 1 + max(1, -(-cfg['end boundary'] // width)))
        self.samples = x[:chunks * width].tolist()
        self.speech_start_index = int(r["start"][0, 0]) if has else 0
        self.speech_end_index = int(r["end"][0, 0]) if has and not is_open else 0
        self.started_speech = is_open
        self.should_end_recording = has and not is_open
        self.cache_data['frame count'] = done
        level, bg = r["level"][0][10:done], r["background"][0][10:done]
        self.levels = level.tolist()
        self.backgrounds = bg.tolist()
        self.final_levels = (level - bg).tolist()
        if len(bg):
            self.cache_data['background'] = float(bg[-1])
        return self

    def start_recording(self, visualize=False):
        """The microphone loop of the reference (record.py:219-241) is not mirrored; it needs `pyaudio`."""
        try:
            import pyaudio  # noqa: F401
        except ImportError:
            raise ImportError("sr.audio_capture: live recording needs the `pyaudio` module, which is not installed; "
                              "AudioRecorder.process(samples) and detect_endpoints(signals) work on recorded audio")
        raise NotImplementedError("sr.audio_capture: the PyAudio microphone loop is not mirrored; "
                                  "use AudioRecorder.process(samples) on recorded audio")

    def _range(self):
        s = self.speech_start_index - self.config['start boundary']
        if s < 0:
            s = 0
        return s, self.speech_end_index

    def get_samples(self, dtype=np.int16):
        s, e = self._range()
        return np.array(self.samples[s:e + 1]).astype(dtype).copy()

    def write_to_wav_file(self, file_name):
        wf = wave.open(file_name, 'wb')
        wf.setnchannels(self.config['channel count'])
        wf.setsampwidth(PA_SAMPLE_WIDTH)
        wf.setframerate(self.config['sample rate'])
        s, e = self._range()
        wf.setnframes(e - s + 1)
        wf.writeframes(np.array(self.samples[s:e + 1]).astype(np.int16).tobytes())
        wf.close()


def record(file=None):
    # make sure the directory that contains the output file exists
    os.makedirs(os.path.dirname(file), exist_ok=True)

    # record
    ar = AudioRecorder()
    ar.start_recording()
    if file:
        ar.write_to_wav_file(file)
    return ar
