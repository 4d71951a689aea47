"""CPU checks of the windowed-streaming entries (uvad_window_*, include/uvad.h): declared in the header, in the ctypes table and exported
by the library; a library built from an older tree is a loud "rebuild" error; and the Python schedule (window_step_plan /
window_schedule) agrees with a brute-force enumeration of the definition in the header."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_window_state_bytes", "uvad_window_workspace_bytes", "uvad_window_reset", "uvad_window_step", "uvad_window_peek",
         "uvad_window_advance", "uvad_window_features"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_window_entries_in_header_binding_and_export_list(built):
    src = _header()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    exported = set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert set(NAMES) <= exported
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", src) and built.ABI_VERSION == 5
    step = built.SIGNATURES["uvad_window_step"]
    assert step[0] is C.c_int and len(step[1]) == 11
    assert built.SIGNATURES["uvad_window_peek"][1][-1] == C.POINTER(C.c_int64)


def test_stale_library_missing_a_symbol_asks_for_a_rebuild(built, monkeypatch):
    sigs = dict(built.SIGNATURES)
    sigs["uvad_window_not_in_this_build"] = (C.c_int, [C.c_void_p])
    monkeypatch.setattr(built, "SIGNATURES", sigs)
    monkeypatch.setattr(built, "_lib", None)
    with pytest.raises(RuntimeError, match="rebuild the library"):
        built.load()


def _brute(chunks, W, L, frame_len=400, shift=160):
    """The header's definition, frame by frame: frame t is complete once samples [t*shift - n_left, t*shift - n_left + frame_len)
    have all arrived; after a step with e complete frames the window is [max(0, e - W), e) and the emitted frames are those below
    e - L not emitted before."""
    n_left = (frame_len - shift) // 2
    if chunks[0] < n_left:
        raise ValueError("first chunk")
    rows, n, emitted = [], 0, 0
    for chunk in chunks:
        n += chunk
        e = 0
        while e * shift - n_left + frame_len <= n:
            e += 1
        hi = max(emitted, e - L)
        rows.append((hi - emitted, max(0, e - W), e, emitted, hi))
        emitted = hi
    return rows


def _check_rows(got, W, L):
    # the window reaches steady state and then emits every new frame exactly once, L frames behind the newest
    assert got[-1][1] == got[-1][2] - W and got[-1][4] == got[-1][2] - L
    assert sum(r[0] for r in got) == got[-1][4]
    for k, lo, hi, e0, e1 in got:
        assert lo <= e0 <= e1 <= hi and hi - lo <= W


@pytest.mark.parametrize("chunk", [320, 250, 1600, 100])
@pytest.mark.parametrize("L", [0, 7, 50])
def test_window_schedule_equals_brute_force_enumeration(chunk, L):
    from uvad_amd.runtime import window_schedule, window_step_plan
    W = 80
    steps = 40 * 1600 // chunk
    if chunk < 120:   # shorter than n_left = (400 - 160) / 2: refused as a first chunk, as by uvad_stream_step
        with pytest.raises(ValueError, match="first chunk"):
            _brute([chunk] * steps, W, L)
        with pytest.raises(ValueError, match="first chunk"):
            window_schedule(steps, chunk, W, L)
        # ... and fine after a longer first one; steps that complete no frame emit nothing
        chunks = [400] + [chunk] * steps
        got, n, e = [], 0, 0
        for c in chunks:
            n, e, row = window_step_plan(n, e, c, W, L)
            got.append(row)
        assert got == _brute(chunks, W, L)
        assert any(r[0] == 0 and r[2] > W for r in got)
        _check_rows(got, W, L)
        return
    got = window_schedule(steps, chunk, W, L)
    assert got == _brute([chunk] * steps, W, L)
    _check_rows(got, W, L)


def test_window_schedule_refusals():
    from uvad_amd.runtime import window_schedule, window_step_plan
    with pytest.raises(ValueError, match="first chunk"):
        window_step_plan(0, 0, 119, 80, 0)
    window_step_plan(0, 0, 120, 80, 0)                     # n_left = 120 samples: the shortest first chunk
    with pytest.raises(ValueError, match="lookahead"):
        window_schedule(2, 320, 10, 8)                     # 8 + 320 // 160 + 1 = 11 > 10
    assert window_schedule(1, 320, 11, 8)[0][0] == 0
    with pytest.raises(ValueError, match="lookahead"):
        window_schedule(1, 320, 80, -1)


def test_window_kernels_keep_the_feature_kernels_memory_discipline():
    """The ring / window kernels run beside the classifier's MFMA kernels: global memory operations only (no FLAT, no LDS), no scratch."""
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindow_stream\.hip\b", mk, re.M)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S",
                          os.path.join(csrc, "window_stream.hip"), "-o", "-"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    isa = out.stdout
    assert "window_assemble_kernel" in isa and "window_emit_kernel" in isa
    assert not re.search(r"^\s+(flat|scratch)_", isa, re.M)
    assert not re.search(r"^\s+ds_", isa, re.M)
    assert not re.search(r"ScratchSize: [1-9]", isa)
