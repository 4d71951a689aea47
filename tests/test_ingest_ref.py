"""CPU checks behind tests/test_gpu_ingest_ratios.py: the derived bound holds for the kernel's arithmetic restated on the CPU
(ingest_ref.chain_f32) on exactly the inputs the GPU accuracy tests feed the kernel, so a GPU failure there is the kernel's; the tap
design and the plan for the rates of the general phase loop (up in {4, 5, 8}) and of the shrunken tiles; the refusals just above the
tap limit; the helpers themselves (tile mirror, random tables, impulse response)."""
import numpy as np
import pytest

import ingest_ref as ref

_ID = lambda k: f"{k[0]}-{k[1]}-x{k[2]}"   # noqa: E731


@pytest.mark.parametrize("key", ref.DESIGNED_CASES + ref.TABLE_CASES, ids=_ID)
def test_the_cpu_chain_is_within_the_derived_bound_of_float64_on_the_gpu_tests_inputs(key):
    case = ref.accuracy_case(key)
    up, down, width = case["up"], case["down"], case["width"]

    def row(b, c):
        x = ref.decode(case["raw"][b, :case["lengths"][b], c], case["encoding"])
        return ref.chain_f32(x, case["taps"], up, down, width)

    worst = ref.check_rows(case, row)
    assert len(case["lengths"]) >= 12 and max(case["lengths"]) * up >= 3 * case["TJ"] * up * down
    print(f"{key[0]} {key[1]} x{key[2]}: {up}/{down} K {case['K']} TJ {case['TJ']}, CPU chain worst error / bound = {worst:.3f}")


def test_the_case_lists_hold_every_named_rate_table_channel_count_and_encoding():
    assert sorted(ref.RATIO_RATES) == [2000, 4000, 6000, 9600, 10000, 12000, 12800, 14000, 20000, 22000, 28000, 40000, 64000]
    for rate, (up, down) in ref.RATIO_RATES.items():
        assert (rate, "int16", 1) in ref.DESIGNED_CASES and (rate, "int16", 3) in ref.DESIGNED_CASES
        assert ref.taps_f64(rate)[1:3] == (up, down)
    assert any(c == 8 for _, _, c in ref.DESIGNED_CASES)
    for enc in ("ulaw", "f32"):
        ups = {ref.RATIO_RATES[r][0] for r, e, _ in ref.DESIGNED_CASES if e == enc}
        assert {4, 5, 8} <= ups, (enc, ups)
    want = {"a": (6000, 8, 3, 30, 63), "b": (6400, 5, 2, 31, 64), "c": (32000, 1, 2, 31, 64), "d": (8000, 2, 1, 31, 63),
            "e": (12000, 4, 3, 0, 3), "f": (2000, 8, 1, 0, 1)}
    for name, (rate, up, down, width, K) in want.items():
        taps, r, u, d, w = ref.table(name)
        assert (r, u, d, w) == (rate, up, down, width) and taps.shape == (up, K) and taps.dtype == np.float32
        assert rate * up == 16000 * down
        assert (name, "int16", 1) in ref.TABLE_CASES and (name, "int16", 3) in ref.TABLE_CASES


@pytest.mark.parametrize("rate", sorted(ref.RATIO_RATES) + [6400])
def test_resample_taps_and_ingest_plan_for_the_new_rates(rate):
    from uvad_amd.ingest import ingest_plan, resample_taps
    taps, up, down, width = resample_taps(rate)
    want, nu, nd, nw = ref.taps_f64(rate)
    assert (up, down, width) == (nu, nd, nw) and (up, down) == ref.RATIO_RATES.get(rate, (5, 2))
    assert taps.shape == want.shape == (up, 2 * width + down) and taps.dtype == np.float32
    assert np.abs(taps.astype(np.float64) - want).max() <= 2.0 ** -24 * np.abs(want).max() * 1.01     # the f32 rounding of the f64 design
    lengths = [0, 1, 2, 3, down - 1, down, down + 1] + np.random.default_rng(rate).integers(0, 100000, 40).tolist()
    plan = ingest_plan(rate, lengths)
    assert (plan["up"], plan["down"], plan["width"], plan["taps_per_phase"]) == (up, down, width, taps.shape[1])
    assert plan["delay"] == ref.delay(up, down, width) and plan["delay"] % up == 0
    assert plan["history"] == plan["delay"] // up * down + width
    for n, m in zip(lengths, plan["lengths"]):
        assert m == ref.out_len(n, up, down) and ((m - 1) * down < n * up <= m * down or n == m == 0)
        if n < 2000:
            assert len(ref.resample_f64(np.zeros(n), taps, up, down, width)) == m == len(ref.chain_f32(np.zeros(n), taps, up, down, width))
    dj, reach = plan["delay"] // up, taps.shape[1] - 1 - width
    # group j of a stream reads input up to (j - dj) down + reach, and holds input up to j down + down - 1 when it runs: the delay keeps
    # a step out of the future.  It is the least such delay or one group more (10 kHz: width 7, down 5 -- 3 groups where 2 would do)
    assert -dj * down + reach <= down - 1 < -(dj - 2) * down + reach


def test_64_khz_is_the_last_rate_under_the_tap_limit_and_80_and_96_khz_are_refused_by_message():
    from uvad_amd.ingest import resample_taps
    taps, up, down, width = resample_taps(64000)
    assert (up, down, width, taps.shape) == (1, 4, 25, (1, 54))
    with pytest.raises(ValueError, match=r"80000 -> 16000 Hz needs 1 phases x 67 taps.*limit of 8 phases x 64 taps"):
        resample_taps(80000)
    with pytest.raises(ValueError, match=r"96000 -> 16000 Hz needs 1 phases x 80 taps.*limit of 8 phases x 64 taps"):
        resample_taps(96000)


def test_tile_mirror_values_worked_by_hand():
    """(C span + up K + C H + C) 4 bytes against 48 KiB, span = (TJ - 1) down + K, worked by hand for the cases the GPU tests lean on."""
    assert ref.tiling(2, 1, 15, 2) == 512 and ref.tiling(5, 3, 17, 1) == 208 and ref.tiling(8, 3, 63, 3) == 128
    assert ref.tiling(1, 3, 41, 8) == 256           # 48 kHz x 8: 1024 -> 99.6 KB, 512 -> 50.4 KB, 256 -> 25.8 KB
    assert ref.tiling(1, 4, 54, 8) == 256           # 64 kHz x 8: 512 -> 67.2 KB, 256 -> 34.4 KB
    assert ref.tiling(2, 5, 41, 8) == 256           # 40 kHz x 8: 512 -> 83.4 KB, 256 -> 42.4 KB
    assert ref.tiling(1, 2, 28, 8) == 512           # 32 kHz x 8: 1024 -> 66.4 KB, 512 -> 33.6 KB
    assert ref.tiling(4, 3, 17, 5) == 256           # 12 kHz x 5: 15.7 KB, no shrink
    assert ref.tiling(1, 4, 54, 8, H=53) == 256 and ref.tiling(8, 3, 63, 2, H=63) == 128
    assert ref.tiling(1, 1, 2 * 31 + 1, 1, H=8 * 1024) == 8192        # a history longer than a tile raises the tile to hold it


def test_random_taps_carry_full_weight_and_chain_equals_an_explicit_loop():
    t = ref.random_taps(5, 64, seed=3)
    assert t.dtype == np.float32 and t.shape == (5, 64) and (np.abs(t) >= 0.25).all() and (np.abs(t) <= 1.0).all()
    assert (t < 0).any() and (t > 0).any() and not np.array_equal(t, t[:, ::-1]) and np.array_equal(t, ref.random_taps(5, 64, seed=3))
    up, down, width = 5, 2, 3
    taps = ref.random_taps(up, 2 * width + down, seed=4)
    x = ref.decode(ref.random_source("int16", (23,), seed=5), "int16")
    got = ref.chain_f32(x, taps, up, down, width)
    assert got.dtype == np.float32 and len(got) == ref.out_len(23, up, down)
    for o in range(len(got)):
        j, p = divmod(o, up)
        acc = np.float32(0.0)
        for k in range(taps.shape[1]):
            f = j * down + k - width
            xv = x[f] if 0 <= f < len(x) else 0.0
            acc = np.float32(float(xv) * float(taps[p, k]) + float(acc))
        assert acc.view(np.uint32) == got[o].view(np.uint32), o


def test_impulse_response_is_the_float64_resampler_of_an_impulse():
    taps, rate, up, down, width = ref.table("b")
    n = 40
    for m in ref.impulse_frames(4, down, width, taps.shape[1], n) + [17]:
        x = np.zeros(n)
        x[m] = 0.5
        y = ref.resample_f64(x, taps, up, down, width)
        want, mask = ref.impulse_response(taps, up, down, width, m, len(y))
        assert np.array_equal(want.astype(np.float64), y) and np.array_equal(mask, y != 0), m
        shifted, smask = ref.impulse_response(taps, up, down, width, m, len(y), shift=2 * up)
        assert np.array_equal(shifted[2 * up:], want[:-2 * up]) and not smask[:2 * up].any()
