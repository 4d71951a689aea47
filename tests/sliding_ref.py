"""numpy restatement of sliding-window inference over whole recordings (uvad_sliding_*, include/uvad.h): the window plan, and the
aggregate in a float64 form (the yardstick) and an f32, ascending-j form (what the kernel computes, operation for operation)."""
import numpy as np


def count(T, W, Hf):
    """Windows of a recording of T frames."""
    if T == 0:
        return 0
    if T <= W:
        return 1
    return -(-(T - W) // Hf) + 1


def brute_count(T, W, Hf):
    """The same by laying windows [j Hf, j Hf + W) until every frame t < T is covered."""
    n, covered = 0, 0
    while covered < T:
        covered = min(T, n * Hf + W)
        n += 1
    return n


def windows(T, W, Hf, n=None):
    """[(start frame, valid frames)] of the first n (default: all) windows of a recording of T frames."""
    n = count(T, W, Hf) if n is None else n
    return [(j * Hf, max(0, min(W, T - j * Hf))) for j in range(n)]


def plan(frames, W, Hf):
    counts = [count(int(t), W, Hf) for t in frames]
    return counts, [0] + list(np.cumsum(counts).astype(int))


def _covering(t, T, W, Hf, n):
    return [j for j in range(n) if 0 <= t - j * Hf < max(0, min(W, T - j * Hf))]


def aggregate_f64(win, frames, first, W, Hf, w=None, T_out=None):
    """win (N, W) window probabilities, frames (R,), first (R + 1,) -> (R, T_out) float64: the weighted mean over the covering windows,
    0 past a recording's frames and where no planned window covers."""
    w = np.ones(W, np.float64) if w is None else np.asarray(w, np.float64)
    win = np.asarray(win, np.float64)
    R = len(frames)
    T_out = int(max(frames)) if T_out is None else T_out
    out = np.zeros((R, T_out), np.float64)
    for r in range(R):
        n = first[r + 1] - first[r]
        for t in range(min(int(frames[r]), T_out)):
            js = _covering(t, int(frames[r]), W, Hf, n)
            if js:
                out[r, t] = sum(w[t - j * Hf] * win[first[r] + j, t - j * Hf] for j in js) / sum(w[t - j * Hf] for j in js)
    return out


def aggregate_f32(win, frames, first, W, Hf, w=None, T_out=None):
    """The same in f32, the windows in ascending j, every product, sum and the quotient rounded once."""
    w = np.ones(W, np.float32) if w is None else np.asarray(w, np.float32)
    win = np.asarray(win, np.float32)
    R = len(frames)
    T_out = int(max(frames)) if T_out is None else T_out
    out = np.zeros((R, T_out), np.float32)
    for r in range(R):
        n = first[r + 1] - first[r]
        for t in range(min(int(frames[r]), T_out)):
            num, den = np.float32(0), np.float32(0)
            js = _covering(t, int(frames[r]), W, Hf, n)
            for j in js:
                k = t - j * Hf
                num = np.float32(num + np.float32(w[k] * win[first[r] + j, k]))
                den = np.float32(den + w[k])
            if js:
                out[r, t] = np.float32(num / den)
    return out
