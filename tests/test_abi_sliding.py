"""CPU checks of sliding-window inference over whole recordings (uvad_sliding_*, include/uvad.h): the entry points are declared in the
header, bound in the ctypes table and exported; uvad_sliding_count, runtime.sliding_plan and a brute-force cover agree; every frame is
covered, the last window is longer than W - Hf, and the waveform model's windows hold the frames the plan says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sliding_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_sliding_configure", "uvad_sliding_count", "uvad_sliding_workspace_bytes", "uvad_sliding_wav_workspace_bytes",
         "uvad_sliding_classify", "uvad_sliding_forward", "uvad_sliding_forward_i16", "uvad_sliding_forward_wav",
         "uvad_sliding_forward_wav_i16"]
W = 64
HOPS = [1, 7, W // 4, W - 1, W]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_sliding_entries_in_header_binding_and_export_list(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.ABI_VERSION == 5                                        # entries appended: the number does not move
    for name in NAMES[4:]:
        ret, args = built.SIGNATURES[name]
        assert ret is C.c_int and len(args) == 15, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == 15, name
    assert built.SIGNATURES["uvad_sliding_count"] == (C.c_int64, [C.c_int64, C.c_int, C.c_int])
    assert len(built.SIGNATURES["uvad_sliding_configure"][1]) == 4
    for name in ("uvad_sliding_workspace_bytes", "uvad_sliding_wav_workspace_bytes"):
        assert built.SIGNATURES[name][0] is C.c_size_t and len(built.SIGNATURES[name][1]) == 5
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bsliding\.hip\b", mk, re.M)


@pytest.mark.parametrize("Hf", HOPS)
def test_count_equals_plan_equals_brute_force(built, Hf):
    from uvad_amd.runtime import sliding_count, sliding_plan
    lib = built.load()
    frames = list(range(0, 3 * W + 2))
    counts, first = sliding_plan(frames, W, Hf)
    assert len(counts) == len(frames) and len(first) == len(frames) + 1 and first[0] == 0
    for T, n, f0, f1 in zip(frames, counts, first, first[1:]):
        assert lib.uvad_sliding_count(T, W, Hf) == n == sliding_count(T, W, Hf) == sr.count(T, W, Hf) == sr.brute_count(T, W, Hf), (T, Hf)
        assert f1 - f0 == n
    assert (counts, first) == tuple(sr.plan(frames, W, Hf))
    assert counts[0] == 0 and counts[1] == 1 and counts[W] == 1 and counts[W + 1] == 2


@pytest.mark.parametrize("Hf", HOPS)
def test_every_frame_is_covered_and_the_last_window_is_long(Hf):
    for T in range(0, 3 * W + 2):
        wins = sr.windows(T, W, Hf)
        covered = np.zeros(T, bool)
        for start, n in wins:
            assert 1 <= n <= W and start + n <= T, (T, Hf, start, n)       # never empty, never past the recording
            covered[start:start + n] = True
        assert covered.all(), (T, Hf)
        if T > W:
            assert wins[-1][1] > W - Hf, (T, Hf, wins[-1])
            assert all(n == W for _, n in wins[:-1])
        if len(wins) > 1:                                                  # no window is redundant: the one before the last does not reach T
            assert wins[-2][0] + wins[-2][1] < T


def test_bad_arguments_of_the_pure_functions(built):
    from uvad_amd.runtime import sliding_count
    lib = built.load()
    for args in ((-1, 64, 16), (10, 0, 1), (10, 64, 0), (10, 64, 65)):
        assert lib.uvad_sliding_count(*args) == -1
        with pytest.raises(ValueError):
            sliding_count(*args)
    assert lib.uvad_sliding_count(2 ** 40, 500, 250) == (2 ** 40 - 500 + 249) // 250 + 1


@pytest.mark.parametrize("Hf", HOPS)
def test_waveform_windows_hold_the_frames_the_plan_says(Hf):
    """Window j of a recording of S samples is its samples [J Hf j, J Hf j + S_w) clipped to S: the SincNet frame count of that clip
    (the floor chain of the three conv + pool stages) equals min(W, T - j Hf), T = frames(S)."""
    from uvad_amd.postprocess import SINC_RF_1, SINC_STEP
    from uvad_amd.runtime import wav_frame_geometry
    from uvad_amd.sincnet import SincNet
    J, R = wav_frame_geometry()
    assert (J, R) == (SINC_STEP, SINC_RF_1) == (270, 991)
    S_w = R + J * (W - 1)
    assert SincNet.num_frames(S_w) == W and SincNet.num_frames(S_w - 1) == W - 1
    rng = np.random.default_rng(Hf)
    sizes = [0, R - 1, R, R + 1, S_w - 1, S_w, S_w + 1, S_w + J * Hf - 1, S_w + J * Hf] + [int(v) for v in rng.integers(R, 4 * S_w, 40)]
    for S in sizes:
        T = max(0, int(SincNet.num_frames(S)))
        assert T == (0 if S < R else (S - R) // J + 1)
        for j, (start, n) in enumerate(sr.windows(T, W, Hf)):
            clip = min(S - J * start, S_w)
            assert max(0, int(SincNet.num_frames(clip))) == n == min(W, T - j * Hf), (S, Hf, j)


def test_aggregate_forms_agree_and_weights():
    from uvad_amd.postprocess import sliding_weights
    assert np.array_equal(sliding_weights("rect", W), np.ones(W, np.float32))
    h = sliding_weights("hamming", W)
    assert h.dtype == np.float32 and h.shape == (W,) and h.min() > 0.079 and abs(h.max() - 1.0) < 2e-3 and np.allclose(h, h[::-1], atol=1e-7)
    with pytest.raises(ValueError):
        sliding_weights("hann", W)
    rng = np.random.default_rng(3)
    frames = [23, 64, 65, 150]
    for Hf in (64, 16, 24):
        counts, first = sr.plan(frames, W, Hf)
        win = rng.random((first[-1], W)).astype(np.float32)
        for w in (None, h):
            a64 = sr.aggregate_f64(win, frames, first, W, Hf, w)
            a32 = sr.aggregate_f32(win, frames, first, W, Hf, w)
            K = -(-W // Hf)
            assert np.abs(a32 - a64).max() <= 4 * (K + 1) * 2.0 ** -24
            assert all(np.all(a64[r, frames[r]:] == 0) for r in range(4))
    # hop = window, rect: the windows laid end to end
    counts, first = sr.plan(frames, W, W)
    win = rng.random((first[-1], W)).astype(np.float32)
    a32 = sr.aggregate_f32(win, frames, first, W, W)
    for r, T in enumerate(frames):
        assert np.array_equal(a32[r, :T], win[first[r]:first[r + 1]].ravel()[:T])
