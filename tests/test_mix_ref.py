"""tests/mix_ref.py checked on the CPU: the vectorised restatement against a plain Python loop, the threshold rule, the energy against
math.fsum, and the share of mixed rows."""
import math

import numpy as np

import mix_ref as mr
from lstm_dropout_ref import philox4x32_10

SEED = 0xC0FFEE1234567


def _loop_energy(x, n):
    """The order of include/uvad.h sample by sample: 1024 lane sums, runs of 64 folded, then the 16 run sums."""
    lanes = [0.0] * 1024
    for i in range(n):
        v = float(np.float32(x[i]))
        lanes[(i // 4) % 1024] += v * v
    for base in range(0, 1024, 64):
        o = 32
        while o:
            for t in range(o):
                lanes[base + t] += lanes[base + t + o]
            o //= 2
    w = [lanes[64 * j] for j in range(16)]
    o = 8
    while o:
        for j in range(o):
            w[j] += w[j + o]
        o //= 2
    return w[0] / n if n else 0.0


def _loop_mix(x, lens, bank, first, amp, mix_prob, max_seg, seed, draw):
    """One call, sample by sample, with Python integers for the draws."""
    B, S = x.shape
    out = np.zeros((B, S), np.float32)
    plans = []
    e_clips = [_loop_energy(bank[first[c]:first[c + 1]], int(first[c + 1] - first[c])) for c in range(len(first) - 1)]
    for b in range(B):
        n = int(lens[b])
        w = [int(v) for v in philox4x32_10((b, 0, draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))]
        mixed = w[0] < int(math.floor(float(np.float32(mix_prob)) * 2.0 ** 32))
        q = (w[1] * len(amp)) >> 32
        e_row = _loop_energy(x[b], n)
        out[b, :n] = x[b, :n]
        segs, off = [], 0
        while mixed and off < n and len(segs) < max_seg:
            k = len(segs)
            wk = w if k == 0 else [int(v) for v in philox4x32_10((b, k, draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))]
            clip = (wk[2] * (len(first) - 1)) >> 32
            cnt = min(int(first[clip + 1] - first[clip]), n - off)
            gain = np.float32(0.0) if e_clips[clip] == 0.0 or e_row == 0.0 else np.float32(amp[q] * math.sqrt(e_row / e_clips[clip]))
            for i in range(cnt):
                out[b, off + i] = np.float32(x[b, off + i] + np.float32(gain * bank[first[clip] + i]))
            segs.append((clip, off, cnt, gain))
            off += cnt
        plans.append({"mixed": mixed, "q": q, "segs": segs})
    return out, plans


def test_restatement_matches_a_plain_loop():
    rng = np.random.default_rng(3)
    B, S, lens = 4, 37, [37, 0, 5, 36]
    x = rng.standard_normal((B, S)).astype(np.float32)
    first = np.array([0, 2, 9, 40, 45], np.int64)
    bank = rng.standard_normal(45).astype(np.float32)
    bank[2:9] = 0.0
    amp = mr.amp_table(10, 20, 4)
    seen = set()
    for draw in range(6):
        got = mr.mix(x, lens, bank, first, amp, 0.6, 3, SEED, draw)
        out, plans = _loop_mix(x, lens, bank, first, amp, 0.6, 3, SEED, draw)
        assert np.array_equal(got["out"].view(np.uint32), out.view(np.uint32))
        assert got["plan"].tobytes() == mr.pack_plan(plans, 3).tobytes()
        assert mr.unpack_plan(got["plan"])[0]["segs"] == got["rows"][0]["segs"]
        seen |= {r["mixed"] for r in got["rows"]} | {len(r["segs"]) for r in got["rows"]}
    assert {True, False, 0, 3} <= seen
    for n in (0, 1, 5, 255, 4096, 4097, 9000):
        v = rng.standard_normal(max(n, 1)).astype(np.float32)
        assert mr.energy(v, n) == _loop_energy(v, n), n
    q = (rng.standard_normal(300) * 8000).astype(np.int16)
    assert mr.energy(q) == _loop_energy(q.astype(np.float32) / np.float32(32768.0), 300)


def test_threshold_rule():
    assert mr.threshold(0.0) == 0 and mr.threshold(1.0) == 1 << 32 and mr.threshold(0.5) == 1 << 31
    rows = np.arange(4096)
    assert not mr.mixed_rows(SEED, 0, rows, 0.0).any() and mr.mixed_rows(SEED, 0, rows, 1.0).all()
    w0 = mr.words(SEED, 0, rows, 0)[:, 0]
    assert np.array_equal(mr.mixed_rows(SEED, 0, rows, 0.5), w0 < np.uint32(1 << 31))
    assert mr.words(0, 0, [0], 0)[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]      # the vector of include/uvad.h


def test_energy_against_fsum():
    rng = np.random.default_rng(11)
    for n in (1, 3, 1023, 4096, 4099, 80000):
        x = (rng.standard_normal(n) * rng.uniform(1e-3, 10.0)).astype(np.float32)
        exact = math.fsum(float(v) * float(v) for v in x)        # every product is exact in double
        got = float(mr.energy_sum(x))
        print(n, abs(got - exact) / exact, (n - 1) * 2.0 ** -53)
        assert abs(got - exact) <= (n - 1) * 2.0 ** -53 * exact, n   # the bound of any order over non-negative terms
        assert mr.energy(x) == np.float64(got) / np.float64(n)
    assert mr.energy(np.zeros(10, np.float32)) == 0.0 and mr.energy(np.ones(5, np.float32), 0) == 0.0


def test_share_of_mixed_rows():
    n = 4096
    share = mr.mixed_rows(SEED, 0, np.arange(n), 0.5).mean()
    assert abs(share - 0.5) <= 5 * math.sqrt(0.25 / n)
    assert mr.mixed_rows(SEED, 0, np.arange(n), 0.5).tolist() != mr.mixed_rows(SEED, 1, np.arange(n), 0.5).tolist()
