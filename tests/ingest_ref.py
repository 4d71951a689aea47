"""Float64 restatement of the ingest stage for tests/test_abi_ingest.py and tests/test_gpu_ingest.py (not collected: no test_ prefix).

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
