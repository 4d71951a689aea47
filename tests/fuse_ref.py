"""Numpy restatement of the channel fusion (uvad_fuse, uvad_fuse_pick; include/uvad.h): loops over groups and members, element-wise over a
group's frames, the MEAN / VOTE accumulation in float64 in slot order.  Written from the header's semantics, not from the kernels."""
import numpy as np

MAX, MEAN, VOTE = 0, 1, 2
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def fuse_ref(x, groups, mode=MAX, threshold=0.5, decide=0.5, lens=None, weights=None, T=None, flags=None):
    """x (B, >= T) f32; groups: list of lists of input rows; weights: None or one list per group; lens (B,) or None.
    -> dict(fused (G, T) f32, glens (G,), labels (G, T) u8, best (G, T) u8, stats (N, 4) u64 [, flags (G,) u8]); columns at or past a
    group's length hold 0 and mean "not written".  The loops over groups and members are explicit, in slot order; the loop over a
    group's frames is the element-wise numpy operation on the frame axis, which is the same arithmetic per frame."""
    x = np.asarray(x, np.float32)
    T = x.shape[1] if T is None else T
    thr, dec = np.float32(threshold), np.float32(decide)
    G, N = len(groups), sum(len(g) for g in groups)
    fused = np.zeros((G, T), np.float32)
    labels = np.zeros((G, T), np.uint8)
    best = np.zeros((G, T), np.uint8)
    glens = np.zeros(G, np.int32)
    stats = np.zeros((N, 4), np.uint64)
    out_flags = np.zeros(G, np.uint8)
    j0 = 0
    with np.errstate(all="ignore"):
        for g, rows in enumerate(groups):
            n = [T if lens is None else min(max(int(lens[r]), 0), T) for r in rows]
            w = [np.float32(1.0)] * len(rows) if weights is None else [np.float32(v) for v in weights[g]]
            L = max(n)
            glens[g] = L
            if flags is not None:
                for r in rows:
                    out_flags[g] |= np.uint8(flags[r])
            bv = np.zeros(L, np.float32)                 # the best value so far and its position, -1: no valid member yet
            bi = np.full(L, -1, np.int64)
            acc, W = np.zeros(L, np.float64), np.zeros(L, np.float64)
            for j, r in enumerate(rows):                 # members in slot order
                p = np.zeros(L, np.float32)
                p[:n[j]] = x[r, :n[j]]                   # columns at or past n are not read
                valid = np.arange(L) < n[j]
                # p ranks strictly above the best so far: NaN above everything, nothing above a NaN; ties keep the lower position
                take = valid & ((bi < 0) | (~np.isnan(bv) & (np.isnan(p) | (p > bv))))
                bv[take], bi[take] = p[take], j
                if mode != MAX:
                    v = p.astype(np.float64) if mode == MEAN else np.where(p < thr, 0.0, 1.0)
                    acc = np.where(valid, acc + np.float64(w[j]) * v, acc)
                    W = np.where(valid, W + np.float64(w[j]), W)
            if mode == MAX:
                f = bv
            else:
                f = np.where(W == 0, np.float32(0.0), (acc / np.where(W == 0, 1.0, W)).astype(np.float32)).astype(np.float32)
                f[np.isnan(f)] = QNAN                    # one NaN, whatever sign the sum gave it
            lab = np.where(f < dec, 0, 1).astype(np.uint8)
            fused[g, :L], labels[g, :L], best[g, :L] = f, lab, bi
            for j, r in enumerate(rows):
                k = n[j]
                own = np.where(x[r, :k] < thr, 0, 1)
                stats[j0 + j] += np.array([k, own.sum(), (own == lab[:k]).sum(), (bi[:k] == j).sum()], np.uint64)
            j0 += len(rows)
    out = {"fused": fused, "glens": glens, "labels": labels, "best": best, "stats": stats}
    if flags is not None:
        out["flags"] = out_flags
    return out


def pick_ref(best, groups, table):
    """table: rows (row, index, first_frame, n_frames, first_sample, n_samples).  -> (re-rowed table, picks)."""
    out, picks = [], []
    for rec in table:
        g, f, k = int(rec[0]), int(rec[2]), int(rec[3])
        if g < 0 or g >= len(groups):
            out.append(tuple(rec))
            picks.append(-1)
            continue
        counts = [0] * len(groups[g])
        for t in range(f, f + k):
            b = int(best[g, t])
            if b < len(counts):
                counts[b] += 1
        kk = max(range(len(counts)), key=lambda i: (counts[i], -i))
        out.append((groups[g][kk],) + tuple(rec[1:]))
        picks.append(kk)
    return out, picks
