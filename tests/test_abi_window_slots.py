"""CPU checks of the slot pools (uvad_window_slots_*, uvad_window_wav_slots_*, include/uvad.h): declared in the header, in the ctypes
table and exported by the library; the Python plans (window_slots_plan / wav_window_slots_plan) agree with a brute-force enumeration of
the header's definition; the new kernels keep to global memory; the refusal arithmetic."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_window_slots_state_bytes", "uvad_window_slots_workspace_bytes", "uvad_window_slots_reset", "uvad_window_slots_step",
         "uvad_window_slots_features", "uvad_window_wav_slots_state_bytes", "uvad_window_wav_slots_workspace_bytes",
         "uvad_window_wav_slots_reset", "uvad_window_wav_slots_step", "uvad_window_wav_slots_step_i16", "uvad_window_wav_slots_features"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_slot_entries_in_header_binding_and_export_list(built):
    src = _header()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", src) and built.ABI_VERSION == 5
    assert re.search(r"#define\s+UVAD_SLOT_START\s+1\b", src) and re.search(r"#define\s+UVAD_SLOT_END\s+2\b", src)
    assert (built.SLOT_START, built.SLOT_END) == (1, 2)
    for name in ("uvad_window_slots_step", "uvad_window_wav_slots_step", "uvad_window_wav_slots_step_i16"):
        ret, args = built.SIGNATURES[name]
        assert ret is C.c_int and len(args) == 13, name
    assert len(built.SIGNATURES["uvad_window_wav_slots_reset"][1]) == 8
    assert len(built.SIGNATURES["uvad_window_slots_reset"][1]) == 7


# ---------------------------------------------------------------------------------------------------------------------------------
# the plans against the header's definition, enumerated


def _brute(flags, chunk, L, complete):
    """complete(n, t): frame t of a session is complete after its first n samples.  Emission by sets: a step emits the session's frames
    t with t + L < e (all t < e on its END step) that no earlier step emitted."""
    out, sess, live, nid = [], {}, {}, 0
    for fl in flags:
        row = []
        for b, f in enumerate(fl):
            if f & 1:
                live[b], sess[nid], nid = nid, [0, set()], nid + 1
            if b not in live:
                row.append((-1, 0, 0, 0))
                continue
            sid = live[b]
            sess[sid][0] += chunk
            n = sess[sid][0]
            e = 0
            while complete(n, e):
                e += 1
            due = {t for t in range(e) if f & 2 or t + L < e} - sess[sid][1]
            sess[sid][1] |= due
            if due:
                assert due == set(range(min(due), max(due) + 1))
                row.append((sid, min(due), max(due) + 1, e))
            else:
                row.append((sid, None, None, e))
            if f & 2:
                del live[b]
        out.append(row)
    return out


def _same(plan, brute):
    assert len(plan) == len(brute)
    for prow, brow in zip(plan, brute):
        for p, q in zip(prow, brow):
            assert p[0] == q[0] and p[3] == q[3], (p, q)
            if q[1] is None:
                assert p[2] - p[1] == 0, (p, q)
            else:
                assert (p[1], p[2]) == (q[1], q[2]), (p, q)


def _random_flags(B, steps, seed):
    rng = np.random.default_rng(seed)
    f = np.zeros((steps, B), np.uint8)
    for b in range(B):
        live = False
        for s in range(steps):
            r = rng.random()
            if not live and r < 0.2:
                f[s, b] = 3 if rng.random() < 0.2 else 1        # one-chunk sessions too
                live = f[s, b] == 1
            elif live and r < 0.05:
                f[s, b] = 1                                     # START on a slot that is mid-session
            elif live and r < 0.12:
                f[s, b], live = 2, False
    f[0, 0], f[1, 0] = 1, 2                                     # END during the warm-up / before the first frame
    f[2, 1] = 3
    return f


@pytest.mark.parametrize("chunk", [320, 250, 1600])
@pytest.mark.parametrize("L", [0, 7, 50])
def test_window_slots_plan_equals_brute_force_enumeration(chunk, L):
    from uvad_amd.runtime import window_slots_plan
    W, n_left = 80, 120
    flags = _random_flags(6, 120, seed=chunk * 7 + L)
    plan = window_slots_plan(flags, chunk, W, L)
    _same(plan, _brute(flags, chunk, L, lambda n, t: t * 160 - n_left + 400 <= n))
    assert any(p[2] - p[1] > 0 and p[2] > p[3] - L for row in plan for p in row if p[0] >= 0) or L == 0   # some END flushed


@pytest.mark.parametrize("chunk", [320, 250, 1600])
@pytest.mark.parametrize("L", [0, 7, 50])
def test_wav_window_slots_plan_equals_brute_force_enumeration(chunk, L):
    from uvad_amd.runtime import wav_window_slots_plan
    W, J, R = 80, 270, 991
    flags = _random_flags(6, 160, seed=chunk * 5 + L)
    _same(wav_window_slots_plan(flags, chunk, W, L, J, R), _brute(flags, chunk, L, lambda n, t: J * t + R <= n))


def test_plans_single_session_equals_the_window_schedules():
    """One session from step 0 that never ends is the existing window stream schedule, step for step."""
    from uvad_amd.runtime import wav_window_schedule, wav_window_slots_plan, window_schedule, window_slots_plan
    flags = np.zeros((150, 1), np.uint8)
    flags[0, 0] = 1
    for row, (k, *_, lo, hi) in zip(window_slots_plan(flags, 320, 60, 7), window_schedule(150, 320, 60, 7)):
        assert (row[0][1], row[0][2]) == (lo, hi) or (k == 0 and row[0][2] - row[0][1] == 0)
    for row, (k, _, _, lo, hi, _, _) in zip(wav_window_slots_plan(flags, 320, 60, 7), wav_window_schedule(150, 320, 60, 7)):
        assert (row[0][1], row[0][2]) == (lo, hi) or (k == 0 and row[0][2] - row[0][1] == 0)


def test_refusal_arithmetic():
    from uvad_amd.runtime import wav_window_slots_ld_out, wav_window_slots_plan, window_slots_ld_out, window_slots_plan
    assert window_slots_ld_out(320, 50) == 53 and window_slots_ld_out(250, 7) == 9 and window_slots_ld_out(1600, 0) == 11
    assert wav_window_slots_ld_out(320, 30) == 32 and wav_window_slots_ld_out(270, 0) == 1 and wav_window_slots_ld_out(1600, 7) == 13
    with pytest.raises(ValueError, match="first"):
        window_slots_plan([], 119, 80, 0)                       # every step can be a session's first: chunk >= 120
    window_slots_plan([], 120, 80, 0)
    with pytest.raises(ValueError, match="lookahead"):
        window_slots_plan([], 320, 10, 8)                       # 8 + 3 > 10
    window_slots_plan([], 320, 11, 8)
    with pytest.raises(ValueError, match="lookahead"):
        window_slots_plan([], 320, 80, 80)
    with pytest.raises(ValueError, match="ceil"):
        wav_window_slots_plan([], 271, 5, 4)                    # 4 + 2 > 5
    wav_window_slots_plan([], 270, 5, 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# ISA


def test_slot_kernels_keep_to_global_memory():
    """The slot kernels run beside the MFMA kernels: global memory operations only (no FLAT, no LDS), no scratch."""
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindow_slots\.hip\b", mk, re.M)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S",
                          os.path.join(csrc, "window_slots.hip"), "-o", "-"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    isa = out.stdout
    for k in ("slot_stage_kernel", "slot_assemble_kernel", "slot_emit_kernel"):
        assert k in isa, k
    assert isa.count("wav_slot_assemble_kernel") >= 2                  # the f32 and the int16 instantiations
    assert not re.search(r"^\s+(flat|scratch)_", isa, re.M)
    assert not re.search(r"^\s+ds_", isa, re.M)
    assert re.search(r"ScratchSize: 0", isa) and not re.search(r"ScratchSize: [1-9]", isa)
