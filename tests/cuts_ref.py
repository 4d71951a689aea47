"""A numpy restatement of the speech cuts (uvad_cuts_table / uvad_cuts_gather, include/uvad.h), written from the header's four steps
and independently of uvad_amd.postprocess: plain loops over runs, nothing shared with the kernels' bit strings or closed forms beyond
the definitions themselves.  The GPU tests compare bytes with it; tests/test_cuts_ref.py compares it with three other restatements."""
import numpy as np

CUT_DTYPE = np.dtype([("row", "<i4"), ("index", "<i4"), ("first_frame", "<i4"), ("n_frames", "<i4"),
                      ("first_sample", "<i8"), ("n_samples", "<i8")])      # uvad_cut, 32 bytes
assert CUT_DTYPE.itemsize == 32


def runs(row):
    """[s, c) of the non-zero bytes of one row, in order."""
    out, s = [], None
    for t, v in enumerate(np.asarray(row).tolist()):
        if v and s is None:
            s = t
        elif not v and s is not None:
            out.append((s, t))
            s = None
    if s is not None:
        out.append((s, len(row)))
    return out


def merged(row, pad):
    """Step 2: every run widened by pad on both sides, clipped to the row, merged into its predecessor when it starts at or before the
    predecessor's end."""
    n, out = len(row), []
    for s, c in runs(row):
        lo, hi = max(s - pad, 0), min(c + pad, n)
        if out and lo <= out[-1][1]:
            out[-1][1] = hi
        else:
            out.append([lo, hi])
    return [(lo, hi) for lo, hi in out]


def split(intervals, max_len, min_len):
    """Step 3 as the reference's loop on integers: full pieces while more than max_len frames remain, the rest kept iff longer than min_len."""
    out = []
    for lo, hi in intervals:
        if max_len > 0:
            while hi - lo > max_len:
                out.append((lo, lo + max_len))
                lo += max_len
        if hi - lo > min_len:
            out.append((lo, hi))
    return out


def row_cuts(row, pad, max_len, min_len):
    """One row's pieces as (first_frame, n_frames)."""
    return [(lo, hi - lo) for lo, hi in split(merged(row, pad), max_len, min_len)]


def table(labels, lens, nsamp, S, cfg):
    """labels (B, >= T) uint8, lens (B,) or None (all columns), nsamp (B,) or None (S) -> (table: CUT_DTYPE array, row_first (B + 1,) int32).
    cfg = (pad, max_len, min_len, hop, lead, tail); T = labels.shape[1]."""
    pad, max_len, min_len, hop, lead, tail = (int(v) for v in cfg)
    labels = np.asarray(labels)
    B, T = labels.shape
    rows, first = [], [0]
    for b in range(B):
        n = T if lens is None else min(max(int(lens[b]), 0), T)
        Sb = int(S) if nsamp is None else min(max(int(nsamp[b]), 0), int(S))
        for k, (f, nf) in enumerate(row_cuts(labels[b, :n], pad, max_len, min_len)):
            s0, s1 = max(f * hop - lead, 0), min((f + nf) * hop + tail, Sb)
            rows.append((b, k, f, nf, s0, max(s1 - s0, 0)))
        first.append(len(rows))
    return np.array(rows, dtype=CUT_DTYPE).reshape(-1), np.asarray(first, np.int32)


def gather(src, tab, which, ld_out, out, out_len):
    """src (B, row_stride[, F]); rows [0, len(tab)) of out (rows, ld_out[, F]) and of out_len are overwritten in place: the cut's first
    min(n, ld_out) units, then zeros.  which: "samples" or "frames"."""
    for i, c in enumerate(tab):
        first, n = (int(c["first_sample"]), int(c["n_samples"])) if which == "samples" else (int(c["first_frame"]), int(c["n_frames"]))
        k = min(n, ld_out)
        out[i] = 0
        out[i, :k] = src[int(c["row"]), first:first + k]
        out_len[i] = k
    return out, out_len
