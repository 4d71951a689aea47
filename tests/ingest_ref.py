"""Float64 restatement of the ingest stage for tests/test_abi_ingest.py, tests/test_ingest_ref.py, tests/test_gpu_ingest.py and
tests/test_gpu_ingest_ratios.py (not collected: no test_ prefix).

The tap design is written from the published algorithm of torchaudio.functional.resample (sinc interpolation, Hann window,
lowpass_filter_width 6, rolloff 0.99), independently of uvad_amd.ingest: scalar loops here, array expressions there."""
import audioop
import math

import numpy as np


def taps_f64(rate, target=16000, lowpass_filter_width=6, rolloff=0.99):
    """(taps float64 [new][K], new, orig, width) of the published design."""
    g = math.gcd(rate, target)
    orig, new = rate // g, target // g
    base = min(orig, new) * rolloff
    width = int(math.ceil(lowpass_filter_width * orig / base))
    K = 2 * width + orig
    taps = np.zeros((new, K), np.float64)
    for p in range(new):
        for k in range(K):
            t = (-p / new + (k - width) / orig) * base
            t = max(-lowpass_filter_width, min(lowpass_filter_width, t))
            w = math.cos(t * math.pi / lowpass_filter_width / 2) ** 2
            t *= math.pi
            taps[p, k] = (1.0 if t == 0 else math.sin(t) / t) * w * base / orig
    return taps, new, orig, width


def out_len(n, up, down):
    return -(-(up * n) // down)


def delay(up, down, width):
    return int(math.ceil((width + down - 1) / down)) * up if (up, down) != (1, 1) else 0


def decode(raw, encoding):
    """raw: array of one channel in the source encoding -> float64 samples (G.711 through audioop, then / 32768)."""
    raw = np.ascontiguousarray(raw)
    if encoding == "f32":
        return raw.astype(np.float64)
    if encoding == "int16":
        return raw.astype(np.float64) / 32768.0
    fn = audioop.ulaw2lin if encoding == "ulaw" else audioop.alaw2lin
    return np.frombuffer(fn(raw.astype(np.uint8).tobytes(), 2), dtype="<i2").astype(np.float64) / 32768.0


def resample_f64(x, taps, up, down, width):
    """x float64 (n,), taps [up][K] (the f32 table the kernel was given, any dtype) -> float64 (ceil(up n / down),):
    output j up + p = sum_k x[j down + k - width] taps[p][k], x zero outside [0, n)."""
    x = np.asarray(x, np.float64)
    taps = np.asarray(taps, np.float64)
    n, K = len(x), taps.shape[1]
    m = out_len(n, up, down)
    groups = -(-m // up) if m else 0
    xp = np.concatenate([np.zeros(width), x, np.zeros(groups * down + K)])
    y = np.zeros(groups * up)
    for j in range(groups):
        seg = xp[j * down:j * down + K]
        y[j * up:(j + 1) * up] = taps @ seg
    return y[:m]


def chain_bound(taps, xmax):
    """Per phase: the error bound of a length-K f32 fma chain on exactly representable inputs, (K + 1) 2^-24 sum_k |taps[p][k]| max|x|."""
    taps = np.asarray(taps, np.float64)
    return (taps.shape[1] + 1) * 2.0 ** -24 * np.abs(taps).sum(1) * xmax


def write_wav(path, raw, tag, rate):
    """raw (frames, channels): int16 for tag 1, uint8 codes for tags 6 (A-law) / 7 (mu-law)."""
    import struct
    raw = np.ascontiguousarray(raw)
    ch = raw.shape[1]
    bits = 16 if tag == 1 else 8
    data = raw.astype("<i2" if tag == 1 else np.uint8).tobytes()
    fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits)
    if tag != 1:
        fmt += struct.pack("<H", 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


# ---------------------------------------------------------------------------------------------------------------------------------
# Helpers of tests/test_gpu_ingest_ratios.py and tests/test_ingest_ref.py: the tile mirror, the kernel's arithmetic restated, tables
# whose every tap carries weight, and the shared cases (the CPU tests walk exactly the inputs the GPU tests feed the kernel).

TILE_OUT, LDS_SOFT = 1024, 48 << 10          # outputs per channel and tile before any shrink; the soft LDS limit of a tile


def _round4(v):
    return (v + 3) // 4 * 4


def tiling(up, down, K, C, H=0):
    """TJ, the output groups per tile the library picks (a mirror of its choice, to place lengths on tile edges and to print which
    tile a case ran with; nothing about the kernel is asserted through it).  H: a stream's history per channel, 0 for a dense call."""
    lds = lambda TJ: (C * ((TJ - 1) * down + K) + up * K + C * H + C) * 4   # noqa: E731
    min_tj = _round4(-(-H // down) if H > 0 else 1)
    TJ = max(_round4(-(-TILE_OUT // up)), min_tj)
    while lds(TJ) > LDS_SOFT and TJ > 4 and _round4(TJ // 2) >= min_tj:
        TJ = _round4(TJ // 2)
    return TJ


def chain_f32(x, taps, up, down, width):
    """The kernel's arithmetic on the CPU: every output its own chain over k = 0 .. K - 1 from +0, each step
    float32(float64(x) float64(t) + float64(acc)) -- an fma but for the double rounding, far below chain_bound.  -> float32 (m,)."""
    x = np.asarray(x, np.float64)
    t64 = np.asarray(taps, np.float32).astype(np.float64)
    n, K = len(x), t64.shape[1]
    m = out_len(n, up, down)
    groups = -(-m // up) if m else 0
    xp = np.concatenate([np.zeros(width), x, np.zeros(groups * down + K)])
    acc = np.zeros((groups, up), np.float32)
    base = np.arange(groups) * down
    for k in range(K):
        acc = (xp[base + k][:, None] * t64[None, :, k] + acc.astype(np.float64)).astype(np.float32)
    return acc.reshape(-1)[:m]


def random_taps(up, K, seed):
    """float32 [up][K], |t| in [0.25, 1], random signs, no symmetry: every tap of every phase carries full weight, so a dropped or
    shifted k moves the output by far more than chain_bound."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.25, 1.0, (up, K)).astype(np.float32)
    return np.ascontiguousarray(np.clip(mag, np.float32(0.25), np.float32(1.0)) * rng.choice(np.float32([-1.0, 1.0]), (up, K)))


RATIO_RATES = {4000: (4, 1), 2000: (8, 1), 12000: (4, 3), 6000: (8, 3), 10000: (8, 5), 14000: (8, 7), 9600: (5, 3), 12800: (5, 4),
               20000: (4, 5), 28000: (4, 7), 22000: (8, 11), 40000: (2, 5), 64000: (1, 4)}                # rate: (up, down)
EIGHT_CHANNEL_RATES = [4000, 6000, 9600, 22000, 40000, 64000]
DESIGNED_CASES = ([(r, "int16", c) for r in RATIO_RATES for c in (1, 3)] + [(r, "int16", 8) for r in EIGHT_CHANNEL_RATES] +
                  [(12000, "ulaw", 1), (9600, "ulaw", 3), (10000, "ulaw", 1), (4000, "f32", 3), (12800, "f32", 1), (2000, "f32", 3)])
TABLES = {"a": (6000, 8, 3, 30), "b": (6400, 5, 2, 31), "c": (32000, 1, 2, 31), "d": (8000, 2, 1, 31), "e": (12000, 4, 3, 0),
          "f": (2000, 8, 1, 0)}                                                                              # name: (rate, up, down, width)
TABLE_CASES = [(t, "int16", c) for t in TABLES for c in (1, 3)] + [("b", "ulaw", 2), ("a", "f32", 8)]


def table(name):
    """(taps, rate, up, down, width) of random table `name` of TABLES."""
    rate, up, down, width = TABLES[name]
    return random_taps(up, 2 * width + down, seed=1000 + ord(name)), rate, up, down, width


def random_source(encoding, shape, seed):
    """Full-scale random samples in the encoding: every int16 value / every G.711 code is as likely as any other."""
    rng = np.random.default_rng(seed)
    if encoding in ("ulaw", "alaw"):
        return rng.integers(0, 256, shape).astype(np.uint8)
    q = rng.integers(-32768, 32768, shape).astype(np.int16)
    return q if encoding == "int16" else q.astype(np.float32) / np.float32(32768.0)


def edge_lengths(up, down, width, K, TJ, long_extra=7):
    """Input lengths of one ragged accuracy call: shorter than the filter, around it, output counts m TJ up + d for m in {1, 2} and
    d in {-1, 0, 1, 4} (where up / down cannot produce a count, the nearest count on either side), and one row of more than 3 tiles."""
    lens = [0, 1, 2, width, K - 1, K, K + 1]
    for m in (1, 2):
        for d in (-1, 0, 1, 4):
            target = m * TJ * up + d
            for n in {target * down // up, -(-target * down // up)}:
                lens.append(n)
    lens += np.random.default_rng(TJ * up + down).integers(K + 2, 5 * TJ * down // 2, 5).tolist()        # and some of no special place
    lens.append(-(-(3 * TJ * up + long_extra) * down // up))
    out, seen = [], set()
    for n in lens:
        if n not in seen:
            seen.add(n)
            out.append(n)
    return out


_CASES = {}


def accuracy_case(key):
    """key: (rate, encoding, channels) of DESIGNED_CASES (the designed table of uvad_amd.ingest.resample_taps) or (table name, encoding, channels) of TABLE_CASES -> the shared inputs of that case: {"raw" (B, S, C), "lengths", "taps", "rate", "up",
    "down", "width", "K", "TJ", "want": float64 rows [b][c], "bound": per-sample bounds [b][c]}.  Built once per process."""
    if key in _CASES:
        return _CASES[key]
    which, encoding, channels = key
    if isinstance(which, str):
        taps, rate, up, down, width = table(which)
    else:
        from uvad_amd.ingest import resample_taps                  # the table ingest_configure uploads by default
        rate = which
        taps, up, down, width = resample_taps(rate)
    K = taps.shape[1]
    TJ = tiling(up, down, K, channels)
    lens = edge_lengths(up, down, width, K, TJ, long_extra=8 if channels == 1 else 7)
    raw = random_source(encoding, (len(lens), max(lens), channels), seed=rate + 17 * channels + len(encoding))
    want, bound = [], []
    for b, n in enumerate(lens):
        m = out_len(n, up, down)
        want.append([])
        bound.append([])
        for c in range(channels):
            x = decode(raw[b, :n, c], encoding)
            want[b].append(resample_f64(x, taps, up, down, width))
            xmax = np.abs(x).max() if n else 0.0
            bound[b].append(chain_bound(taps, xmax)[np.arange(m) % up])
    case = {"raw": raw, "lengths": lens, "taps": taps, "rate": rate, "up": up, "down": down, "width": width, "K": K, "TJ": TJ,
            "encoding": encoding, "channels": channels, "want": want, "bound": bound}
    _CASES[key] = case
    return case


def check_rows(case, rows):
    """rows(b, c) -> that row's outputs (at least its count of them).  Every sample of every row within the case's bound of float64:
    none is left out.  Returns worst error / bound."""
    worst = 0.0
    for b, n in enumerate(case["lengths"]):
        m = out_len(n, case["up"], case["down"])
        for c in range(case["channels"]):
            y = np.asarray(rows(b, c), np.float64)[:m]
            err = np.abs(y - case["want"][b][c])
            bd = case["bound"][b][c]
            assert err.shape == (m,) and bd.shape == (m,) and (err <= bd).all(), (b, n, c, float(err.max()), float(bd.max()))
            if m:
                worst = max(worst, float((err / np.maximum(bd, 1e-300)).max()))
    return worst


def impulse_frames(TJ, down, width, K, n):
    """The input frames an impulse test visits: 0, the last frame, and the first, centre and last frame under the first and the last
    output group of tiles 0, 1 and 2."""
    ms = [0, n - 1]
    for j in (0, TJ - 1, TJ, 2 * TJ - 1, 2 * TJ, 3 * TJ - 1):
        ms += [j * down - width, j * down, j * down + K - 1 - width]
    out = []
    for m in ms:
        if 0 <= m < n and m not in out:
            out.append(m)
    return out


def impulse_response(taps, up, down, width, m, n_out, shift=0):
    """float32 (n_out,): the exact output for an input of 0.5 at frame m and zero elsewhere -- output shift + j up + p =
    float32(0.5 taps[p][m - j down + width]) where that index lies in [0, K), zero elsewhere -- and the mask of that support."""
    taps = np.asarray(taps, np.float32)
    K = taps.shape[1]
    want = np.zeros(n_out, np.float32)
    mask = np.zeros(n_out, bool)
    for j in range(max(0, -(-(m + width - K + 1) // down)), (m + width) // down + 1):
        for p in range(up):
            o = shift + j * up + p
            if o < n_out:
                want[o] = np.float32(0.5) * taps[p, m - j * down + width]
                mask[o] = True
    return want, mask
