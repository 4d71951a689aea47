"""Host side of the ingest stage (uvad_ingest*, include/uvad.h): what can be computed without a GPU.

``resample_taps``: the polyphase table the library is handed (it computes none itself).  The default design is the published
Hann-windowed sinc interpolation kernel of torchaudio.functional.resample at its defaults (lowpass_filter_width 6, rolloff 0.99), which
is what lhotse's ``resample`` applies; restated here from the published algorithm.  Parity with lhotse's resampler is unpinned
(torchaudio is not a dependency), as the log-mel stage's parity with lhotse's Fbank is.
``ingest_plan``: output lengths, the stream delay and the history a stream carries.  ``g711_table``: the G.711 expansion tables."""
import math

import numpy as np

ENCODINGS = {"f32": 0, "int16": 1, "ulaw": 2, "alaw": 3}          # UVAD_INGEST_* of include/uvad.h
ENCODING_DTYPES = {"f32": np.float32, "int16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}
MAX_PHASES, MAX_TAPS, MAX_CHANNELS = 8, 64, 8                      # UVAD_INGEST_MAX_PHASES / _MAX_TAPS; channels of uvad_ingest_configure


def resample_ratio(rate: int, target: int = 16000):
    """(up, down) = target / rate reduced."""
    rate, target = int(rate), int(target)
    if rate < 1 or target < 1:
        raise ValueError(f"sample rates must be positive (got {rate}, {target})")
    g = math.gcd(rate, target)
    return target // g, rate // g


def resample_taps(rate: int, target: int = 16000, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(taps float32 [up][K], up, down, width), K = 2 * width + down: output j * up + p = sum_k x[j * down + k - width] * taps[p][k].
    None for taps when up / down = 1 / 1 (no table).  A table beyond 8 phases or 64 taps per phase (44.1 kHz: 160 x 475) is refused."""
    up, down = resample_ratio(rate, target)
    if up == 1 and down == 1:
        return None, 1, 1, 0
    base = min(down, up) * rolloff
    width = int(math.ceil(lowpass_filter_width * down / base))
    K = 2 * width + down
    if up > MAX_PHASES or K > MAX_TAPS:
        raise ValueError(f"resampling {rate} -> {target} Hz needs {up} phases x {K} taps: beyond the limit of {MAX_PHASES} phases x {MAX_TAPS} "
                         "taps per phase")
    idx = np.arange(-width, width + down, dtype=np.float64) / down
    t = (-np.arange(up, dtype=np.float64) / up)[:, None] + idx[None, :]
    t = np.clip(t * base, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    safe = np.where(t == 0, 1.0, t)
    kernel = np.where(t == 0, 1.0, np.sin(safe) / safe) * window * (base / down)
    return np.ascontiguousarray(kernel, np.float32), up, down, width


def stream_delay(up: int, down: int, width: int):
    """(D, H): a stream's output is the dense output delayed by D = ceil((width + down - 1) / down) * up samples; it carries the last
    H = D * down / up + width input samples per row."""
    dj = -(-(width + down - 1) // down) if (up, down) != (1, 1) else 0
    return dj * up, dj * down + width


def ingest_plan(rate: int, lengths, target: int = 16000, width: int = None):
    """{"up", "down", "width", "taps_per_phase", "delay", "history", "lengths"} for input rows of `lengths` samples (an int or a
    sequence): output lengths ceil(up * n / down).  width: of a custom table; default: that of resample_taps."""
    up, down = resample_ratio(rate, target)
    if width is None:
        width = resample_taps(rate, target)[3]
    D, H = stream_delay(up, down, width)
    one = np.isscalar(lengths)
    ns = [int(lengths)] if one else [int(n) for n in lengths]
    if any(n < 0 for n in ns):
        raise ValueError("lengths must be >= 0")
    out = [-(-(up * n) // down) for n in ns]
    return {"up": up, "down": down, "width": width, "taps_per_phase": 2 * width + down if (up, down) != (1, 1) else 1,
            "delay": D, "history": H, "lengths": out[0] if one else out}


def g711_table(encoding: str) -> np.ndarray:
    """int16 [256]: the ITU-T G.711 expansion of every code, "ulaw" or "alaw" (the 16-bit values a wav decoder gives)."""
    out = np.zeros(256, np.int16)
    for code in range(256):
        if encoding == "ulaw":
            u = ~code & 0xFF
            t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
            out[code] = 0x84 - t if u & 0x80 else t - 0x84
        elif encoding == "alaw":
            a = code ^ 0x55
            t = (a & 0x0F) << 4
            seg = (a & 0x70) >> 4
            t = t + 8 if seg == 0 else (t + 0x108) << (seg - 1)
            out[code] = t if a & 0x80 else -t
        else:
            raise ValueError(f"encoding must be 'ulaw' or 'alaw', got {encoding!r}")
    return out
