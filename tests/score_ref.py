"""Plain numpy restatement of the scoring stage (uvad_score_*, uvad_intervals_to_labels, include/uvad.h): median labels at every operating
point, the collar, tp / fp / tn / fn, the probability histogram per class and the binary cross-entropy sum in float64.  Written from the
header's text, independent of the kernels; tests/test_score_ref.py checks it against brute force."""
import math

import numpy as np


def median_labels(p, thr, kernel):
    """p (n,) f32 -> y (n,) bool: x = !(p < thr) (NaN counts as speech), y[t] = sum of x over [t - h, t + h] within [0, n) exceeds h."""
    with np.errstate(invalid="ignore"):
        x = ~(np.asarray(p, np.float32) < np.float32(thr))
    n, h = len(x), kernel // 2
    c = np.concatenate(([0], np.cumsum(x.astype(np.int64))))
    t = np.arange(n)
    return c[np.minimum(t + h + 1, n)] - c[np.maximum(t - h, 0)] > h


def scored_mask(g, collar):
    """g (n,) bool -> (n,) bool: frame t is unscored iff a boundary k in 1 .. n - 1 (g[k - 1] != g[k]) has k - c <= t <= k + c - 1."""
    n = len(g)
    keep = np.ones(n, bool)
    for k in np.flatnonzero(g[1:] != g[:-1]) + 1:
        keep[max(k - collar, 0):min(k + collar, n)] = False
    return keep


def bce_terms(p, g):
    """float64 terms of F.binary_cross_entropy from f32 probabilities: -(g max(log p, -100) + (1 - g) max(log(1 - p), -100))."""
    q = np.where(g, np.asarray(p, np.float32).astype(np.float64), 1.0 - np.asarray(p, np.float32).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.log(q)
    return -np.where(l < -100.0, -100.0, l)          # NaN stays NaN


def hist_bins(p, bins):
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        v = p * np.float32(bins)
        b = np.where(v < bins, np.floor(np.where(np.isnan(v), 0, v)), bins - 1).astype(np.int64)
        b = np.where(np.isnan(v), bins - 1, b)
    return np.clip(b, 0, bins - 1)


def score(probs, gt, lens, points, collar, bins):
    """probs (B, >= T) f32, gt (B, >= T) uint8, lens (B,) (None: full rows) -> dict(counts (P, 4) tp fp tn fn, rows (B, 4) of point 0,
    hist (2, bins), loss_sum (math.fsum of the float64 terms), valid)."""
    B = probs.shape[0]
    T = probs.shape[1]
    lens = [T] * B if lens is None else [min(max(int(v), 0), T) for v in lens]
    counts = np.zeros((len(points), 4), np.int64)
    rows = np.zeros((B, 4), np.int64)
    hist = np.zeros((2, bins), np.int64)
    terms = []
    for b in range(B):
        n = lens[b]
        if n == 0:
            continue
        p, g = probs[b, :n], gt[b, :n] != 0
        keep = scored_mask(g, collar)
        for m, (thr, kernel) in enumerate(points):
            y = median_labels(p, thr, kernel)
            c = np.array([(y & g & keep).sum(), (y & ~g & keep).sum(), (~y & ~g & keep).sum(), (~y & g & keep).sum()], np.int64)
            counts[m] += c
            if m == 0:
                rows[b] = c
        hb = hist_bins(p, bins)
        for cls in (0, 1):
            hist[cls] += np.bincount(hb[keep & (g == bool(cls))], minlength=bins)
        terms.append(bce_terms(p, g))
    flat = np.concatenate(terms) if terms else np.zeros(0)
    loss = float("nan") if np.isnan(flat).any() else math.fsum(flat.tolist())
    return {"counts": counts, "rows": rows, "hist": hist, "loss_sum": loss, "valid": int(sum(lens))}


def intervals_to_labels(iv, iv_counts, T, lens, out):
    """The union of [max(s, 0), min(e, len_b)) over row b's first iv_counts[b] intervals written into out (B, ld) uint8 on [0, len_b);
    bytes at or past len_b stay."""
    out = out.copy()
    for b in range(out.shape[0]):
        n = T if lens is None else min(max(int(lens[b]), 0), T)
        out[b, :n] = 0
        for s, e in np.asarray(iv[b][:max(min(int(iv_counts[b]), len(iv[b])), 0)]).reshape(-1, 2):
            s, e = max(int(s), 0), min(int(e), n)
            if e > s:
                out[b, s:e] = 1
    return out
