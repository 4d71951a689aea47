"""CPU checks of the causal stream's slot pool (uvad_stream_slots_*, include/uvad.h): declared in the header, in the ctypes table and
exported by the library; uvad_stream_slots_kmax is ceil(chunk / shift); the closed-form plan (stream_slots_plan) agrees with the
brute-force frame loop of tests/stream_ref.py under a schedule of staggered starts, restarts and one-chunk sessions; the refusal
arithmetic that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stream_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_stream_slots_kmax", "uvad_stream_slots_state_bytes", "uvad_stream_slots_workspace_bytes", "uvad_stream_slots_reset",
         "uvad_stream_slots_step"]
CHUNKS = (160, 250, 320, 480, 560, 640)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_stream_slot_entries_in_header_binding_and_export_list(built):
    src = _header()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    # the step has uvad_window_slots_step's argument list: whatever drives one drives the other
    assert built.SIGNATURES["uvad_stream_slots_step"] == built.SIGNATURES["uvad_window_slots_step"]
    ret, args = built.SIGNATURES["uvad_stream_slots_step"]
    assert ret is C.c_int and len(args) == 13
    assert len(built.SIGNATURES["uvad_stream_slots_reset"][1]) == 5
    assert built.SIGNATURES["uvad_stream_slots_kmax"] == (C.c_int, [C.c_void_p, C.c_int])
    assert built.SIGNATURES["uvad_stream_slots_state_bytes"][0] is C.c_size_t
    assert built.SIGNATURES["uvad_stream_slots_workspace_bytes"][0] is C.c_size_t
    decl = re.search(r"int\s+uvad_stream_slots_step\s*\(([^;]*)\)\s*;", src).group(1)
    ref = re.search(r"int\s+uvad_window_slots_step\s*\(([^;]*)\)\s*;", src).group(1)
    assert re.sub(r"\s+", " ", decl) == re.sub(r"\s+", " ", ref)


def test_kmax_is_ceil_chunk_over_shift(built):
    """ceil(chunk / frame_shift) for chunks 120 .. 700: the Python restatement the runtime sizes its buffers with, against a frame loop
    (the most frames any step of a long feed completes); the library's entry refuses a missing context.  (A context needs a device:
    uvad_stream_slots_kmax itself is held to the same numbers in tests/test_gpu_stream_slots.py.)"""
    from uvad_amd.runtime import stream_slots_kmax
    lib = built.load()
    for chunk in range(120, 701):
        assert stream_slots_kmax(chunk, 160) == -(-chunk // 160) == (chunk + 159) // 160
        assert max(sr.k_schedule(chunk, 24)) <= stream_slots_kmax(chunk), chunk
    assert [stream_slots_kmax(c) for c in CHUNKS] == [1, 2, 2, 3, 4, 4]
    assert [max(sr.k_schedule(c, 60)) for c in CHUNKS] == [1, 2, 2, 3, 4, 4]          # attained
    assert lib.uvad_stream_slots_kmax(None, 320) < 0
    assert lib.uvad_stream_slots_state_bytes(None, 7) == 0 and lib.uvad_stream_slots_workspace_bytes(None, 7, 320) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan against the frame loop


def _schedule(B, steps, seed):
    """Staggered starts within one tile, END then START in the next step, START | END, START on an active slot, a slot idle for many
    steps before its first START, a slot that is never started, END on an idle slot."""
    rng = np.random.default_rng(seed)
    f = np.zeros((steps, B), np.uint8)
    for b in range(B - 2):
        live = False
        for s in range(steps):
            r = rng.random()
            if not live and r < 0.25:
                f[s, b] = 3 if rng.random() < 0.25 else 1
                live = f[s, b] == 1
            elif live and r < 0.06:
                f[s, b] = 1
            elif live and r < 0.14:
                f[s, b], live = 2, False
    f[:, 0] = 0
    f[0, 0], f[3, 0], f[4, 0], f[5, 0], f[6, 0] = 1, 2, 1, 3, 1       # END then START next step; a one-chunk session; restart
    f[:, 1] = 0
    f[1, 1], f[2, 1] = 1, 1                                          # START on an active slot
    f[:, B - 2] = 0
    f[steps // 2, B - 2] = 1                                         # idle for many steps before its first START
    f[:, B - 1] = 0
    f[2, B - 1] = 2                                                  # END on an idle slot: nothing
    return f


def _brute(flags, chunk):
    """Per step and slot (session, lo, hi, frames) from the frame loop: a session that holds n samples has sr.frames_complete(n) frames."""
    out, sess, live, nid = [], {}, {}, 0
    for fl in flags:
        row = []
        for b, f in enumerate(fl):
            if f & 1:
                live[b], sess[nid], nid = nid, [0, 0], nid + 1
            if b not in live:
                row.append((-1, 0, 0, 0))
                continue
            sid = live[b]
            sess[sid][0] += chunk
            e_prev, e = sess[sid][1], sr.frames_complete(sess[sid][0])
            sess[sid][1] = e
            row.append((sid, e_prev, e, e))
            if f & 2:
                del live[b]
        out.append(row)
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
def test_stream_slots_plan_equals_the_frame_loop(chunk):
    from uvad_amd.runtime import stream_slots_kmax, stream_slots_plan
    flags = _schedule(7, 90, seed=chunk)
    plan, brute = stream_slots_plan(flags, chunk), _brute(flags, chunk)
    assert len(plan) == len(brute) == 90
    counts = set()
    for prow, brow in zip(plan, brute):
        for p, q in zip(prow, brow):
            assert p[0] == q[0] and p[3] == q[3], (p, q)
            assert p[2] - p[1] == q[2] - q[1] and (p[2] == p[1] or (p[1], p[2]) == (q[1], q[2])), (p, q)
            assert 0 <= p[2] - p[1] <= stream_slots_kmax(chunk)
            if p[0] >= 0:
                counts.add(p[2] - p[1])
    assert stream_slots_kmax(chunk) in counts                      # the bound is attained
    assert all(p[0] == -1 for row in plan for p in row[-1:])       # the never-started slot stays idle, END on it included
    assert all(row[5][0] == -1 for row in plan[:45]) and plan[45][5][0] >= 0


def test_one_session_is_the_lockstep_stream_schedule():
    from uvad_amd.runtime import stream_slots_plan
    for chunk in CHUNKS:
        flags = np.zeros((60, 1), np.uint8)
        flags[0, 0] = 1
        assert [r[0][2] - r[0][1] for r in stream_slots_plan(flags, chunk)] == sr.k_schedule(chunk, 60)


def test_refusal_arithmetic():
    from uvad_amd.runtime import STREAM_SLOTS_KMAX, stream_slots_kmax, stream_slots_plan
    assert STREAM_SLOTS_KMAX == 4
    assert stream_slots_kmax(640) == 4 and stream_slots_kmax(641) == 5 and stream_slots_kmax(160) == 1 and stream_slots_kmax(161) == 2
    with pytest.raises(ValueError, match="first"):
        stream_slots_plan([], 119)                                 # every step can be a session's first: chunk >= 120
    stream_slots_plan([], 120)
    with pytest.raises(ValueError, match="ceil"):
        stream_slots_plan([], 641)                                 # 5 frames in one step
    stream_slots_plan([], 640)
    with pytest.raises(ValueError, match="ceil"):
        stream_slots_plan([], 400, 400, 80)                        # the limit follows the geometry: 5 shifts of 80
    stream_slots_plan([], 320, 400, 80)
