"""A restatement of the hysteresis decisions (uvad_binarize, include/uvad.h), written from the header's six steps as loops over frames
and runs: nothing shared with the kernel's bit words, carry chains or prefix maxima, nor with uvad_amd.postprocess, beyond the
definitions themselves.  The GPU tests compare bytes with it; tests/test_binarize_ref.py compares it with other restatements."""
from collections import namedtuple

import numpy as np

Cfg = namedtuple("Cfg", "onset offset min_on min_off pad_on pad_off")


def cfg(onset=0.5, offset=None, min_on=0, min_off=0, pad_on=0, pad_off=0):
    return Cfg(float(onset), float(onset if offset is None else offset), int(min_on), int(min_off), int(pad_on), int(pad_off))


def states(p, n, q):
    """Steps 1 and 2: the 0/1 state of frames [0, n).  The comparisons are made in f32, the type of the probabilities and of the record."""
    p = np.asarray(p, np.float32)
    on, off = np.float32(q.onset), np.float32(q.offset)
    s, st = [], 0
    for t in range(n):
        v = p[t]
        if not (v < on):
            st = 1
        elif v < off:
            st = 0
        s.append(st)
    return s


def runs_of(s):
    """Step 3: [start, stop) of the 1s of a list, in order."""
    out, a = [], None
    for t, v in enumerate(s):
        if v and a is None:
            a = t
        elif not v and a is not None:
            out.append((a, t))
            a = None
    if a is not None:
        out.append((a, len(s)))
    return out


def row(p, n, q):
    """One row's kept intervals [(lo, hi)]: pad, then fill, then drop."""
    out = []
    for a, c in runs_of(states(p, n, q)):
        lo, hi = max(a - q.pad_on, 0), min(c + q.pad_off, n)
        if out and (lo - out[-1][1] <= 0 or lo - out[-1][1] < q.min_off):
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return [(lo, hi) for lo, hi in out if hi - lo >= q.min_on]


def batch(probs, lens, q):
    """probs (B, >= T) f32, lens (B,) or None (all columns) -> per-row interval lists; T = probs.shape[1]."""
    probs = np.asarray(probs)
    B, T = probs.shape
    return [row(probs[b], T if lens is None else min(max(int(lens[b]), 0), T), q) for b in range(B)]


def labels_of(intervals, n):
    """(n,) uint8: 1 on the union of the intervals."""
    lab = np.zeros(n, np.uint8)
    for lo, hi in intervals:
        for t in range(lo, hi):
            lab[t] = 1
    return lab


def outputs(probs, lens, q, max_iv, labels, iv, counts):
    """What uvad_binarize leaves in labels (B, ld) uint8 (or None), iv (B, max_iv, 2) int32 and counts (B,) int32, written over copies
    of the arrays given: bytes the call does not write keep what they held."""
    probs = np.asarray(probs)
    B, T = probs.shape
    labels = None if labels is None else labels.copy()
    iv, counts = iv.copy(), counts.copy()
    for b, ivs in enumerate(batch(probs, lens, q)):
        n = T if lens is None else min(max(int(lens[b]), 0), T)
        counts[b] = len(ivs)
        for k, (lo, hi) in enumerate(ivs[:max_iv]):
            iv[b, k] = lo, hi
        if labels is not None:
            labels[b, :n] = labels_of(ivs, n)
    return labels, iv, counts
