"""CPU restatement of the noise-mixing stage (uvad_mix_*, include/uvad.h): the energies in the documented order, the draws through
lstm_dropout_ref.philox4x32_10, the plan of every row, the gains and the mixed output, to the bit."""
import numpy as np

from lstm_dropout_ref import philox4x32_10

LANES, RUN = 1024, 64            # lanes of the energy order, and the run of lanes folded first
PLAN_HEAD, SEG_WORDS = 4, 4      # int32 words of a plan row: {mixed, q, nseg, 0} + {clip, dst offset, count, gain bits} per segment


def amp_table(lo, hi, Q):
    """The noise-to-speech amplitude ratios of Q SNR steps over lo .. hi dB, as the Python layer fills them."""
    return np.array([10 ** (-(lo + (hi - lo) * (q + 0.5) / Q) / 20) for q in range(Q)], np.float64)


def threshold(mix_prob):
    """floor(mix_prob 2^32) for mix_prob given as an f32: 0 .. 2^32."""
    return int(np.floor(float(np.float32(mix_prob)) * 4294967296.0))


def to_f32(x):
    """The samples as the device reads them: f32 as they are, int16 as q / 32768."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(1.0 / 32768.0)
    assert x.dtype == np.float32, x.dtype
    return x


def energy_sum(x, n=None):
    """sum (double)x (double)x over the first n samples in the order of include/uvad.h: lane t = (i / 4) mod 1024 adds its samples in
    increasing i; within each run of 64 lanes t += t + o for o = 32 .. 1; the 16 run sums j += j + o for o = 8 .. 1."""
    x = to_f32(x).reshape(-1)
    n = len(x) if n is None else int(n)
    if n <= 0:
        return np.float64(0.0)
    v = x[:n].astype(np.float64)
    sq = v * v
    pad = -n % (4 * LANES)
    a = np.concatenate([sq, np.zeros(pad)]).reshape(-1, LANES, 4)          # [pass][lane][sample of the group]; +0 changes no sum >= +0
    acc = np.zeros(LANES)
    with np.errstate(all="ignore"):
        for p in range(a.shape[0]):
            for e in range(4):
                acc = acc + a[p, :, e]
        w = acc.reshape(LANES // RUN, RUN).copy()
        o = RUN // 2
        while o:
            w[:, :o] = w[:, :o] + w[:, o:2 * o]
            o //= 2
        r = w[:, 0].copy()
        o = len(r) // 2
        while o:
            r[:o] = r[:o] + r[o:2 * o]
            o //= 2
        return r[0]


def energy(x, n=None):
    """E(x, n) = energy_sum / n: one division; 0 for n = 0."""
    n = np.asarray(x).size if n is None else int(n)
    with np.errstate(all="ignore"):
        return energy_sum(x, n) / np.float64(n) if n > 0 else np.float64(0.0)


def clip_energies(bank, clip_first):
    return np.array([energy(bank[clip_first[i]:clip_first[i + 1]]) for i in range(len(clip_first) - 1)], np.float64)


def words(seed, draw, rows, k):
    """The four Philox words of (row, segment k): counter (row, k, draw_lo, draw_hi), key (seed_lo, seed_hi) -> (len(rows), 4) uint32."""
    rows = np.asarray(rows, np.uint64) & np.uint64(0xFFFFFFFF)
    out = philox4x32_10((rows, np.full(len(rows), k, np.uint64), draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1)


def mixed_rows(seed, draw, rows, mix_prob):
    """The decision of every row: (uint64)w0 < floor(mix_prob 2^32)."""
    return words(seed, draw, rows, 0)[:, 0].astype(np.uint64) < np.uint64(threshold(mix_prob))


def plan(e_rows, lens, clip_first, e_clips, amp, mix_prob, max_seg, seed, draw, row0=0):
    """-> list of dicts {mixed, q, segs: [(clip, offset, count, gain f32)]}, one per row."""
    clip_first = [int(v) for v in clip_first]
    n_clips, Q = len(clip_first) - 1, len(amp)
    out = []
    for b, n in enumerate(lens):
        row = (row0 + b) & 0xFFFFFFFF
        w = words(seed, draw, [row], 0)[0]
        mixed = int(w[0]) < threshold(mix_prob)
        q = (int(w[1]) * Q) >> 32
        segs, off = [], 0
        while mixed and off < n and len(segs) < max_seg:
            wk = w if not segs else words(seed, draw, [row], len(segs))[0]
            clip = (int(wk[2]) * n_clips) >> 32
            cnt = min(clip_first[clip + 1] - clip_first[clip], n - off)
            gain = np.float32(0.0)
            if e_clips[clip] != 0.0 and e_rows[b] != 0.0:
                with np.errstate(all="ignore"):
                    gain = np.float32(np.float64(amp[q]) * np.sqrt(np.float64(e_rows[b]) / np.float64(e_clips[clip])))
            segs.append((clip, off, cnt, gain))
            off += cnt
        out.append({"mixed": bool(mixed), "q": q, "segs": segs})
    return out


def pack_plan(rows, max_seg):
    """The plan record d_plan [B][4 + 4 max_seg] int32."""
    out = np.zeros((len(rows), PLAN_HEAD + SEG_WORDS * max_seg), np.int32)
    for b, r in enumerate(rows):
        out[b, :3] = (int(r["mixed"]), r["q"], len(r["segs"]))
        for k, (clip, off, cnt, gain) in enumerate(r["segs"]):
            out[b, PLAN_HEAD + SEG_WORDS * k:PLAN_HEAD + SEG_WORDS * (k + 1)] = (clip, off, cnt, int(np.float32(gain).view(np.int32)))
    return out


def unpack_plan(words_):
    """The inverse of pack_plan for one batch (used to apply the device's own plan)."""
    rows = []
    for r in np.asarray(words_, np.int32):
        segs = [(int(r[PLAN_HEAD + SEG_WORDS * k]), int(r[PLAN_HEAD + SEG_WORDS * k + 1]), int(r[PLAN_HEAD + SEG_WORDS * k + 2]),
                 r[PLAN_HEAD + SEG_WORDS * k + 3:PLAN_HEAD + SEG_WORDS * k + 4].view(np.float32)[0]) for k in range(int(r[2]))]
        rows.append({"mixed": bool(r[0]), "q": int(r[1]), "segs": segs})
    return rows


def apply(x, lens, bank, clip_first, rows):
    """out = fl32(x + fl32(gain noise)) inside the segments, the input's bits outside, +0 past a length."""
    x = to_f32(x)
    out = x.copy()
    bank = np.asarray(bank, np.float32)
    with np.errstate(all="ignore"):
        for b, r in enumerate(rows):
            out[b, int(lens[b]):] = 0.0
            for clip, off, cnt, gain in r["segs"]:
                nz = bank[int(clip_first[clip]):int(clip_first[clip]) + cnt]
                out[b, off:off + cnt] = x[b, off:off + cnt] + (np.float32(gain) * nz).astype(np.float32)
    return out


def lengths(B, S, nsamp=None):
    return np.full(B, S, np.int64) if nsamp is None else np.clip(np.asarray(nsamp, np.int64), 0, S)


def mix(x, nsamp, bank, clip_first, amp, mix_prob, max_seg, seed, draw, row0=0, e_clips=None):
    """One uvad_mix_apply call -> dict(out (B, S) f32, plan (B, 4 + 4 max_seg) int32, e_rows, e_clips, rows)."""
    x = np.asarray(x)
    B, S = x.shape
    lens = lengths(B, S, nsamp)
    e_rows = np.array([energy(x[b], lens[b]) for b in range(B)], np.float64)
    e_clips = clip_energies(bank, clip_first) if e_clips is None else e_clips
    rows = plan(e_rows, lens, clip_first, e_clips, amp, mix_prob, max_seg, seed, draw, row0)
    return {"out": apply(x, lens, bank, clip_first, rows), "plan": pack_plan(rows, max_seg), "e_rows": e_rows, "e_clips": e_clips, "rows": rows}
