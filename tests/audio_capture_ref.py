# -*- coding: utf-8 -*-
"""Numpy restatement of the endpoint detection of AudioRecorder (sr/audio_capture/record.py:78-91, 116-217, 243-248)
for the tests: what `record_callback` computes when it is fed whole chunks of `samples per frame` samples, as a function
of a recorded signal -- vectorised energies, then the classifier as a Python loop over frames, in the reference's order
of operations.  `max_segments` > 1 re-arms the detector after an end with every piece of state left as it is (the
extension csrc/gh_endpoint.hip implements); `max_segments = 1` is the reference.  Test-only."""
import numpy as np

DEFAULT_CONFIG = {
    'sample rate': 8000, 'format': 8, 'chunk size': 1024, 'channel count': 1, 'forget factor': 1,
    'max record time': 1000, 'frame time': 0.02, 'frame stride': 0.01, 'adjustment': 0.01, 'onset threshold': 3,
    'offset threshold': 0.2, 'silence threshold': 500, 'speech threshold': 250, 'start boundary': 200, 'end boundary': 0,
}


def derive(config):
    """record.py:78-91 on a COPY of `config`: widths, thresholds and boundaries in samples / frames."""
    c = dict(config)
    c['samples per frame'] = int(c['frame time'] * c['sample rate'])
    c['frame stride'] = int(c['frame stride'] * c['sample rate'])
    c['silence threshold'] = int(c['silence threshold'] * c['sample rate'] / (1000 * c['frame stride']))
    c['speech threshold'] = int(c['speech threshold'] * c['sample rate'] / (1000 * c['frame stride']))
    c['start boundary'] = int(c['start boundary'] / 1000 * c['sample rate'])
    c['end boundary'] = int(c['end boundary'] / 1000 * c['sample rate'])
    return c


def frame_count(n_samples, width, stride):
    """Frames the callback appends for n_samples // width whole chunks: one for the first, int(width / stride) for
    every later one (record.py:132-147)."""
    chunks = n_samples // width
    return 0 if chunks == 0 else 1 + int(width / stride) * (chunks - 1)


def energies(signal, width, stride):
    """calc_energy (record.py:23-31) of every frame; frame 0 is never classified and keeps energy 0."""
    nf = frame_count(len(signal), width, stride)
    if nf == 0:
        return np.zeros(0)
    cs = np.concatenate([[0], np.cumsum(np.asarray(signal, dtype=np.int64) ** 2)])
    first = np.arange(nf, dtype=np.int64) * stride
    s = cs[first + width] - cs[first]
    e = np.where(s <= 1, 0.0, 10 * np.log10(np.maximum(s, 2)))
    e[0] = 0.0
    return e


def detect(signal, cfg, max_segments=1):
    """cfg: a DERIVED config.  Returns a dict: start / end (lists, one entry per segment, an open segment's end is
    len(signal) - 1), open, is_speech [nf] (the frames' attribute), level / background / energy [nf] (zero where the
    reference computes nothing), levels / backgrounds / final_levels (the reference's debug lists), frames_done
    (frames the classifier went through: the one at which it stopped included), margin (smallest distance of a
    compared `level - background` from 0, onset and offset; inf without any comparison), clamped_while_carrying
    (frames that took the clamp branch while a speech decision was carried: attribute and returned decision differ)."""
    width, stride = cfg['samples per frame'], cfg['frame stride']
    ff, adj = cfg['forget factor'], cfg['adjustment']
    onset, offset = cfg['onset threshold'], cfg['offset threshold']
    E = energies(signal, width, stride)
    nf = len(E)
    attr = np.zeros(nf, dtype=bool)
    level = np.zeros(nf)
    background = np.zeros(nf)
    energy = np.zeros(nf)
    levels, backgrounds, finals = [], [], []
    starts, ends = [], []
    bg = 0
    speech = silence = 0
    started = False
    margin = np.inf
    clamped_carry = 0
    done = min(nf, 1)
    for i in range(1, nf):
        done = i + 1
        e = E[i]
        energy[i] = e
        is_speech = False
        if i <= 10:
            level[i] = e
        else:
            level[i] = (level[i - 1] + (ff * e)) / (ff + 1)
            is_speech = bool(attr[i - 1])
        if i >= 10:
            if i == 10:
                for f in range(11):
                    bg += E[f]
                bg /= 10
            else:
                bg += (e - bg) * adj
            d = level[i] - bg
            if not (d == 0 and e == 0):
                margin = min(margin, abs(d), abs(d - onset), abs(d - offset))
            if level[i] < bg:
                level[i] = bg
                clamped_carry += is_speech          # attribute False, returned decision True: the two part ways here
            elif level[i] - bg > onset:
                attr[i] = True
                is_speech = True
            elif level[i] - bg < offset:
                attr[i] = False
                is_speech = False
            else:
                attr[i] = is_speech
            background[i] = bg
            finals.append(level[i] - bg)
            levels.append(level[i])
            backgrounds.append(bg)
        if is_speech:
            speech += 1
            silence = 0
        else:
            silence += 1
            speech = 0
        if speech > cfg['speech threshold'] and not started:
            silence = 0
            started = True
            starts.append(i * stride)
        elif silence > cfg['silence threshold'] and started:
            started = False
            ends.append(i * stride + width)
            if len(ends) == max_segments:
                break
    is_open = started
    if is_open:
        ends.append(len(signal) - 1)
    return dict(start=starts, end=ends, open=is_open, is_speech=attr, level=level, background=background, energy=energy,
                levels=np.array(levels), backgrounds=np.array(backgrounds), final_levels=np.array(finals),
                frames_done=done, margin=margin, clamped_while_carrying=clamped_carry)


def get_samples_range(start, end, n_samples, start_boundary):
    """The slice of get_samples (record.py:243-248) for the reference's two indices, as (begin, stop)."""
    return max(start - start_boundary, 0), min(end + 1, n_samples)
