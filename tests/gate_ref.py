"""A plain-loop restatement of the live speech gate's step rule (uvad_gate_*, include/uvad.h), written from the header and sharing nothing
with uvad_amd: one label at a time, samples by their positions.  tests/test_gate_ref.py proves it against tests/cuts_ref.py's table + gather on
whole sessions; the GPU tests compare every step's bytes with it."""
import numpy as np

START, END = 1, 2                              # the flag bits of a step (UVAD_SLOT_START / UVAD_SLOT_END)
FIRST, LAST, LOST, SHORT = 1, 2, 4, 8          # UVAD_GATE_*
INT_MAX = 2 ** 31 - 1
SEG_DTYPE = np.dtype([("index", "<i4"), ("flags", "<i4"), ("first_frame", "<i4"), ("n_frames", "<i4"), ("offset", "<i8"),
                      ("n", "<i4"), ("n_stored", "<i4")])                  # uvad_gate_seg, 32 bytes
assert SEG_DTYPE.itemsize == 32
IDLE, OPEN, PENDING = 0, 1, 2


def history(cfg, lag, chunk):
    """uvad_gate_history: chunk + (lag + pad + 1) hop + lead."""
    pad, max_len, min_len, hop, lead, tail = cfg
    return chunk + (lag + pad + 1) * hop + lead


def max_seg(cfg, ld_lab):
    """uvad_gate_max_seg."""
    pad, max_len, min_len, hop, lead, tail = cfg
    iv = (ld_lab + 1) // 2 + 1
    return min(2 * iv + 1 + ((ld_lab + 2 * pad * iv) // max_len if max_len else 0), INT_MAX)


def max_out(cfg, ld_lab, chunk):
    """uvad_gate_max_out."""
    pad, max_len, min_len, hop, lead, tail = cfg
    iv = (ld_lab + 1) // 2 + 1
    return chunk + (ld_lab + 2 * pad * iv) * hop + max_seg(cfg, ld_lab) * (lead + tail)


class Slot:
    """One slot, step by step.  cfg = (pad, max_len, min_len, hop, lead, tail) with min_len = 0; hist: samples the ring holds."""

    def __init__(self, cfg, hist, dtype=np.int16):
        self.pad, self.W, min_len, self.hop, self.lead, self.tail = (int(v) for v in cfg)
        assert min_len == 0
        self.H, self.dtype = int(hist), np.dtype(dtype)
        self.ring = np.zeros(self.H, self.dtype)
        self.wp = 0                 # the ring's write position: it runs on across sessions
        self.live = False
        self._clear()
        self.trace = set()          # which situations this slot has met (the tests' self-check reads it)

    def _clear(self):
        self.A = self.F = 0                     # samples and labels of the session so far
        self.mode, self.c = IDLE, 0
        self.pf = self.idx = self.sent = 0      # the current piece: first frame, cut index, samples delivered so far
        self.started = False                    # ... and whether it has a record yet

    # -- records -----------------------------------------------------------------------------------------------------------------------
    def _record(self, flags, k, upto):
        """The current piece, k frames so far, delivers its samples up to the absolute position `upto`."""
        first = max(self.pf * self.hop - self.lead, 0)
        total = max(upto - first, 0)
        n = total - self.sent
        assert n >= 0
        if not (flags & LAST) and n == 0:
            return                                                          # an open piece with nothing new says nothing
        src = first + self.sent
        if not self.started:
            flags |= FIRST
        if n > 0 and src < self.A - self.H:
            flags |= LOST
        self.recs.append((self.idx, flags, self.pf, k, self.sent, n, src))
        self.sent, self.started = total, True

    def _close(self, k, ending):
        """The current piece closes with k frames: the rest of its samples, LAST."""
        want = (self.pf + k) * self.hop + self.tail
        flags = LAST | (SHORT if (not ending and self.A < want) else 0)
        if k < self.W or not self.W:
            self.trace.add("last piece")
        self._record(flags, k, min(want, self.A))
        self.idx += 1
        self.pf += k
        self.sent, self.started = 0, False

    def _cover(self, g, ending):
        """Frames below g are known to lie inside the interval: every piece they complete closes."""
        while self.W and g - self.pf >= self.W:
            self.trace.add("split")
            self._close(self.W, ending)

    def _known(self):
        return self.F if self.mode == OPEN else min(self.c + self.pad, self.F)

    # -- a step ------------------------------------------------------------------------------------------------------------------------
    def step(self, chunk, labels, flags, ld_out, max_seg_):
        """chunk: this step's samples; labels: the labels finalised by this step -> (out (ld_out,), seg array of min(count, max_seg)
        records, the true count).  An idle slot reads neither and returns nothing."""
        out = np.zeros(ld_out, self.dtype)
        self.recs = []
        if flags & START:
            if self.live:
                self.trace.add("restart without END")
            self._clear()
            self.live = True
        if not self.live:
            return out, np.zeros(0, SEG_DTYPE), 0
        ending = bool(flags & END)
        if flags & START and ending:
            self.trace.add("one-step session")
        chunk = np.asarray(chunk, self.dtype)                               # commit the chunk, then read
        self.ring[(self.wp + np.arange(len(chunk))) % self.H] = chunk
        self.wp = (self.wp + len(chunk)) % self.H
        self.A += len(chunk)
        for v in np.asarray(labels).tolist():
            if self.F >= INT_MAX:
                break                                                       # the frame counter saturates
            t, v = self.F, bool(v)
            if self.mode == IDLE and v:
                self.pf, self.mode = max(t - self.pad, 0), OPEN
            elif self.mode == OPEN and not v:
                self.c, self.mode = t, PENDING
            elif self.mode == PENDING and v:
                self.mode = OPEN
                self.trace.add("rejoin")
            self.F = t + 1
            if self.mode == PENDING and not v and t >= self.c + 2 * self.pad:
                hi = self.c + self.pad
                self._cover(hi, ending)
                if hi > self.pf:
                    self._close(hi - self.pf, ending)
                self.mode = IDLE
            elif self.mode != IDLE:
                self._cover(self._known(), ending)
        if self.mode != IDLE:
            if ending:
                self.trace.add("ended open" if self.mode == OPEN else "ended pending")
                hi = self._known()
                self._cover(hi, True)
                if hi > self.pf:
                    self._close(hi - self.pf, True)
            else:
                g = self._known()
                if g > self.pf:
                    self._record(0, g - self.pf, min(g * self.hop, self.A))
        # the records -> the output row
        seg, off = [], 0
        for r, (idx, fl, f, k, offset, n, src) in enumerate(self.recs):
            if r >= max_seg_:
                break
            ns = min(n, ld_out - off)
            if fl & (FIRST | LAST) == FIRST | LAST and n == 0:
                self.trace.add("empty piece")
            p = src + np.arange(ns)                                         # sample p sits A - p places behind the write position
            at = (self.wp - (self.A - p)) % self.H
            held = p >= self.A - self.H
            out[off:off + ns] = np.where(held, self.ring[at], 0)
            if held.any() and at[held][0] > at[held][-1]:
                self.trace.add("ring wrap")
            seg.append((idx, fl, f, k, offset, n, ns))
            off += ns
        count = len(self.recs)
        if ending:
            self._clear()
            self.live = False
        return out, np.array(seg, SEG_DTYPE).reshape(-1), count


def simulate(cfg, hist, chunks, labels, lab_counts, flags, ld_out, max_seg_):
    """chunks (steps, B, chunk), labels (steps, B, ld_lab), lab_counts (steps, B), flags (steps, B) -> out[step][slot] = Slot.step's
    triple, and the slots (for their traces)."""
    steps, B = flags.shape
    slots = [Slot(cfg, hist, chunks.dtype) for _ in range(B)]
    ld_lab = labels.shape[2]
    res = [[slots[b].step(chunks[s, b], labels[s, b, :max(0, min(int(lab_counts[s, b]), ld_lab))], int(flags[s, b]), ld_out, max_seg_)
            for b in range(B)] for s in range(steps)]
    return res, slots


def assemble(records):
    """[(seg record, its samples)] of one session, in order -> {index: (first_frame, n_frames, flags or-ed, samples)}; asserts the
    fragments of a cut arrive in order, back to back, with FIRST on the first and LAST on the last."""
    cuts, order = {}, []
    for r, data in records:
        i = int(r["index"])
        if i not in cuts:
            assert r["flags"] & FIRST and r["offset"] == 0, r
            assert not order or cuts[order[-1]]["done"], "a cut began before its predecessor's LAST"
            assert i == len(order), "cut indices count up from 0"
            cuts[i] = {"first_frame": int(r["first_frame"]), "flags": 0, "parts": [], "len": 0, "done": False, "n_frames": 0}
            order.append(i)
        else:
            assert not r["flags"] & FIRST, r
        c = cuts[i]
        assert not c["done"] and r["first_frame"] == c["first_frame"] and r["offset"] == c["len"] and r["n_frames"] >= c["n_frames"], r
        assert len(data) == r["n_stored"]
        c["parts"].append(np.asarray(data))
        c["len"] += int(r["n"])
        c["flags"] |= int(r["flags"])
        c["n_frames"] = int(r["n_frames"])
        c["done"] = bool(r["flags"] & LAST)
    return [(cuts[i]["first_frame"], cuts[i]["n_frames"], cuts[i]["flags"], np.concatenate(cuts[i]["parts"]), cuts[i]["done"]) for i in order]
