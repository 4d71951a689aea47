"""numpy restatement of the live endpointer (uvad_endpoint_*, include/uvad.h), written for the tests: a session's whole probability row ->
its median labels (by counting) and its merged, padded interval list; and a step-wise simulator that says which labels and events every
step must produce, whatever the cut of the frames into steps."""
import numpy as np

START, END = 1, 2          # event kinds; also the flag bits of a step (UVAD_SLOT_START / UVAD_SLOT_END)


def threshold(p, thr=0.5):
    """x[t] = !(p[t] < thr) in float32: NaN counts as speech."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        return (~(p < np.float32(thr))).astype(np.uint8)


def median_labels(x, K):
    """Binary median of odd length K = 2 h + 1 over the 0/1 row x, zeros outside it: y[t] = 1 iff more than h of x[t - h .. t + h] are 1."""
    x = np.asarray(x, np.int64)
    h, n = K // 2, len(x)
    cs = np.concatenate(([0], np.cumsum(x)))
    t = np.arange(n)
    ones = cs[np.minimum(t + h + 1, n)] - cs[np.maximum(t - h, 0)]
    return (ones > h).astype(np.uint8)


def runs(y):
    """[(first speech frame, first non-speech frame after it)] of a 0/1 row; a run open at the end closes at len(y)."""
    d = np.diff(np.concatenate(([0], np.asarray(y, np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def merged(y, P):
    """The runs of y widened by P frames on both sides, clipped to [0, len(y)], an interval merging into its predecessor when its start
    is <= the predecessor's end."""
    n, out = len(y), []
    for s, c in runs(y):
        lo, hi = max(s - P, 0), min(c + P, n)
        if out and lo <= out[-1][1]:
            out[-1][1] = hi
        else:
            out.append([lo, hi])
    return [tuple(v) for v in out]


def whole(p, K, P, thr=0.5):
    """A session's whole row -> (labels uint8 (n,), [(lo, hi)])."""
    y = median_labels(threshold(p, thr), K)
    return y, merged(y, P)


def events_of(intervals):
    out = []
    for lo, hi in intervals:
        out += [(START, lo), (END, hi)]
    return out


class Slot:
    """One slot of the endpointer, step by step.  It keeps the session's thresholded frames and applies the streaming rules as the header
    states them: y[t] is final once frame t + h is there (or at END); START when a final 1 meets no open or pending interval; a run closed
    at c is pending until y[c .. c + 2 P] are final and zero, then END at c + P; a 1 at s <= c + 2 P rejoins; the END flag closes at
    min(c + P, n), or at n in speech."""

    def __init__(self, K, P, thr=0.5):
        self.K, self.h, self.P, self.thr = K, K // 2, P, thr
        self._clear()

    def _clear(self):
        self.x, self.fin, self.state, self.c = [], 0, "idle", 0

    def step(self, p, flags=0):
        """p: this step's probabilities (n_b of them) -> (labels finalised by the step, [(kind, frame)], active)."""
        if flags & START:
            self._clear()
        self.x += threshold(p, self.thr).tolist()
        m = len(self.x)
        upto = m if flags & END else max(0, m - self.h)
        y = median_labels(self.x, self.K)[self.fin:upto] if upto > self.fin else np.zeros(0, np.uint8)
        ev = []
        for t, v in enumerate(y.tolist(), self.fin):
            if self.state == "idle" and v:
                ev.append((START, max(t - self.P, 0)))
                self.state = "speech"
            elif self.state == "speech" and not v:
                self.state, self.c = "pending", t
            elif self.state == "pending" and v:
                self.state = "speech"
            if self.state == "pending" and not v and t >= self.c + 2 * self.P:
                ev.append((END, self.c + self.P))
                self.state = "idle"
        self.fin = max(self.fin, upto)
        if flags & END:
            if self.state == "speech":
                ev.append((END, m))
            elif self.state == "pending":
                ev.append((END, min(self.c + self.P, m)))
            self._clear()
        return y, ev, int(self.state != "idle")


def simulate(probs, counts, flags, K, P, thr=0.5):
    """probs (steps, B, ld_in), counts (steps, B), flags (steps, B) -> out[step][slot] = (labels, events, active)."""
    steps, B = counts.shape
    slots = [Slot(K, P, thr) for _ in range(B)]
    return [[slots[b].step(probs[s, b, :max(0, min(int(counts[s, b]), probs.shape[2]))], int(flags[s, b])) for b in range(B)] for s in range(steps)]


def sessions(counts, flags):
    """[(slot, first step, last step, ended)] of a schedule; the frames before a slot's first START belong to a session that began at
    reset (first step 0)."""
    steps, B = flags.shape
    out = []
    for b in range(B):
        s0 = 0
        for s in range(steps):
            if flags[s, b] & START and s > s0:
                out.append((b, s0, s - 1, False))
            if flags[s, b] & START:
                s0 = s
            if flags[s, b] & END:
                out.append((b, s0, s, True))
                s0 = s + 1
        if s0 < steps:
            out.append((b, s0, steps - 1, False))
    return out


def session_row(probs, counts, b, s0, s1):
    """The frames slot b consumed in steps s0 .. s1, concatenated."""
    parts = [probs[s, b, :max(0, min(int(counts[s, b]), probs.shape[2]))] for s in range(s0, s1 + 1)]
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)
