"""CPU restatement of the reverberation stage (uvad_reverb_*, include/uvad.h): the draws through lstm_dropout_ref.philox4x32_10, the delays,
the plan of every row, the convolution in float64 (np.convolve), the energies of mix_ref.py, the gain and the output."""
import numpy as np

from lstm_dropout_ref import philox4x32_10
from mix_ref import energy, lengths, to_f32

PLAN_WORDS = 4                    # int32 words of a plan row: {applied, r, d, gain bits}
WORD1 = 0x52560000                # word 1 of every counter of this stage
ONE_BITS = int(np.float32(1.0).view(np.int32))


def threshold(prob):
    """floor(prob 2^32) for prob given as an f32: 0 .. 2^32."""
    return int(np.floor(float(np.float32(prob)) * 4294967296.0))


def words(seed, draw, rows):
    """The four Philox words of every row: counter (row, 0x52560000, draw_lo, draw_hi), key (seed_lo, seed_hi) -> (len(rows), 4) uint32."""
    rows = np.asarray(rows, np.uint64) & np.uint64(0xFFFFFFFF)
    out = philox4x32_10((rows, np.full(len(rows), WORD1, np.uint64), draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1)


def taps(first, max_taps=0):
    """K_r of every response: its length, or min(length, max_taps) when max_taps > 0."""
    k = np.diff(np.asarray(first, np.int64))
    return np.minimum(k, max_taps) if max_taps > 0 else k


def delay(h):
    """The smallest k at which |h[k]| is largest; a NaN never wins (a response of NaNs: 0)."""
    best, at = -1.0, 0
    for k, v in enumerate(np.abs(np.asarray(h, np.float32))):
        if v > best:              # False for a NaN
            best, at = float(v), k
    return at


def delays(bank, first, max_taps=0):
    K = taps(first, max_taps)
    return np.array([delay(bank[int(first[r]):int(first[r]) + int(K[r])]) for r in range(len(K))], np.int32)


def plan(B, n_rirs, dly, prob, align, seed, draw, row0=0):
    """-> (B, 4) int32 {applied, r, d, bits of 1.0f}: the record before the gains are known."""
    w = words(seed, draw, [(row0 + b) & 0xFFFFFFFF for b in range(B)])
    out = np.zeros((B, PLAN_WORDS), np.int32)
    out[:, 3] = ONE_BITS
    for b in range(B):
        if int(w[b, 0]) < threshold(prob):
            r = (int(w[b, 1]) * n_rirs) >> 32
            out[b, :3] = (1, r, int(dly[r]) if align else 0)
    return out


def conv64(x, h, d):
    """z[i] = sum_k h[k] x[i + d - k] for 0 <= i < len(x), x outside its range 0, in float64.  The chain of the device starts from +0, so
    a sum of zeros is +0: adding +0.0 turns a -0 of np.convolve into it."""
    n = len(x)
    if n == 0:
        return np.zeros(0, np.float64)
    full = np.convolve(np.asarray(x, np.float64), np.asarray(h, np.float64))
    z = np.zeros(n, np.float64)
    m = max(0, min(n, len(full) - d))
    z[:m] = full[d:d + m]
    return z + 0.0


def bound(x, h, d):
    """sum_k |h[k]| |x[i + d - k]| per sample, in float64: what the rigorous error bound of a K-term f32 sum scales with."""
    return conv64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(h, np.float64)), d)


def gain(x, z, n):
    """g = (float)sqrt(E_in / E_out) over the f32 values of x and z; 1.0f when either energy is 0."""
    e_in, e_out = energy(x, n), energy(np.asarray(z, np.float32), n)
    if e_in == 0.0 or e_out == 0.0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        return np.float32(np.sqrt(np.float64(e_in) / np.float64(e_out)))


def scale(z, g):
    """out = fl32(z g): one rounding."""
    with np.errstate(all="ignore"):
        return (np.asarray(z, np.float32) * np.float32(g)).astype(np.float32)


def reverb(x, nsamp, bank, first, prob, normalize, align, max_taps, seed, draw, row0=0, z_dev=None):
    """One uvad_reverb_apply call -> dict(out (B, S) f32, plan (B, 4) int32, z64: {row: float64 z}, absbound: {row: sum |h||x|}).
    out rounds the float64 z to f32 once: it is what the device gives bit for bit only where every partial sum is exact (integer
    operands).  z_dev: the device's own z (B, S) f32 -- the gain and the output are then restated from its bits."""
    x = np.asarray(x)
    B, S = x.shape
    lens = lengths(B, S, nsamp)
    xf = to_f32(x)
    K, dly = taps(first, max_taps), delays(bank, first, max_taps)
    pl = plan(B, len(K), dly, prob, align, seed, draw, row0)
    out = xf.copy()
    z64, absb = {}, {}
    for b in range(B):
        n = int(lens[b])
        out[b, n:] = 0.0
        if not pl[b, 0]:
            continue
        r, d = int(pl[b, 1]), int(pl[b, 2])
        h = np.asarray(bank, np.float32)[int(first[r]):int(first[r]) + int(K[r])]
        z64[b] = conv64(xf[b, :n], h, d)
        absb[b] = bound(xf[b, :n], h, d)
        z = z64[b].astype(np.float32) if z_dev is None else np.asarray(z_dev, np.float32)[b, :n]
        if normalize:
            g = gain(xf[b], z, n)
            pl[b, 3] = int(g.view(np.int32))
            z = scale(z, g)
        out[b, :n] = z
    return {"out": out, "plan": pl, "z64": z64, "absbound": absb, "lens": lens}
