"""A step-wise simulator of the live hysteresis endpointer (uvad_endpoint_hyst_*, include/uvad.h), written from the header's six
streaming rules as a loop over frames: one slot, one frame at a time, nothing shared with the kernel's ballot words, carry chain or
count-trailing-zeros jumps.  The offline answer it is compared against is tests/binarize_ref.py."""
import numpy as np

import binarize_ref as br

START, END = 1, 2          # event kinds; also the flag bits of a step (UVAD_SLOT_START / UVAD_SLOT_END)
IDLE, SPEECH, PENDING = 0, 1, 2


def lag(q):
    """uvad_endpoint_hyst_lag: min_on + D, the most labels a slot can owe."""
    return q.min_on + gap(q)


def gap(q):
    """D: raw runs at most this far apart end in one interval."""
    return q.pad_on + q.pad_off + max(q.min_off - 1, 0)


class Slot:
    """One slot, step by step.  labels: the session's labels final so far, [0, F)."""

    def __init__(self, q):
        self.q, self.D = q, gap(q)
        self._clear()

    def _clear(self):
        self.m, self.s, self.mode, self.conf, self.lo, self.c, self.F = 0, 0, IDLE, False, 0, 0, 0

    def _fill(self, out, value, upto):
        """Labels [F, upto) become final with one value."""
        if upto > self.F:
            out += [value] * (upto - self.F)
            self.F = upto

    def _frame(self, v, out, ev):
        q, t = self.q, self.m
        on, off = np.float32(q.onset), np.float32(q.offset)
        # 1 the state bit, compared in f32
        if not (v < on):
            self.s = 1
        elif v < off:
            self.s = 0
        # 2 the mode
        if self.mode == IDLE and self.s:
            self.lo, self.mode, self.conf = max(t - q.pad_on, 0), SPEECH, False
        elif self.mode == SPEECH and not self.s:
            self.c, self.mode = t, PENDING
        elif self.mode == PENDING and self.s:
            self.mode = SPEECH
        # 3 close
        if self.mode == PENDING and not self.s and t >= self.c + self.D:
            hi = self.c + q.pad_off
            if self.conf:
                ev.append((END, hi))
            self._fill(out, 1 if self.conf else 0, hi)       # [lo, hi): kept or dropped
            self.mode, self.conf = IDLE, False
        # 4 confirm
        self.m = m = t + 1
        if self.mode != IDLE and not self.conf:
            bound = m if self.mode == SPEECH else min(self.c + q.pad_off, m)
            if bound - self.lo >= q.min_on:
                ev.append((START, self.lo))
                self.conf = True
        # 5 the frontier
        if self.mode == IDLE:
            self._fill(out, 0, m - q.pad_on)
        elif self.conf and self.mode == SPEECH:
            self._fill(out, 1, m)
        elif self.conf:
            self._fill(out, 1, min(self.c + q.pad_off, m))

    def step(self, p, flags=0):
        """p: this step's probabilities (n_b of them) -> (labels finalised by the step, [(kind, frame)], active byte)."""
        if flags & START:
            self._clear()
        out, ev = [], []
        with np.errstate(invalid="ignore"):
            for v in np.asarray(p, np.float32):
                self._frame(v, out, ev)
        if flags & END:                                       # 6
            n = self.m
            if self.mode != IDLE:
                hi = n if self.mode == SPEECH else min(self.c + self.q.pad_off, n)
                if self.conf:
                    ev.append((END, hi))
                    self._fill(out, 1, hi)
            self._fill(out, 0, n)
            self._clear()
        active = 0 if self.mode == IDLE else 1 if self.conf else 2
        return np.array(out, np.uint8), ev, active

    @property
    def backlog(self):
        return self.m - self.F


def simulate(probs, counts, flags, q):
    """probs (steps, B, ld_in), counts (steps, B), flags (steps, B) -> out[step][slot] = (labels, events, active)."""
    steps, B = counts.shape
    slots = [Slot(q) for _ in range(B)]
    return [[slots[b].step(probs[s, b, :max(0, min(int(counts[s, b]), probs.shape[2]))], int(flags[s, b])) for b in range(B)] for s in range(steps)]


def events_of(intervals):
    out = []
    for lo, hi in intervals:
        out += [(START, lo), (END, hi)]
    return out


def whole(p, q):
    """A session's whole row -> (labels uint8 (n,), [(lo, hi)]) by the offline restatement."""
    iv = br.row(p, len(p), q)
    return br.labels_of(iv, len(p)), iv
