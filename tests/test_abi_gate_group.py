"""CPU checks of the group gate's entry points (uvad_gate_group_*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; the size helpers against their formulas (tests/gate_group_ref.py) and -1 / 0 on bad arguments; every refusal, all of which are
made before the library touches a device; UVAD_E_STATE before uvad_fuse_configure; and the pools' group_gate= keyword.  Without a GPU
uvad_fuse_configure validates, keeps the configuration and then fails its upload with UVAD_E_HIP, which is what lets the refusals be
checked here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import gate_group_ref as gg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"uvad_gate_group_history": 4, "uvad_gate_group_best_history": 4, "uvad_gate_group_max_out": 4, "uvad_gate_group_state_bytes": 5,
         "uvad_gate_group_reset": 9, "uvad_gate_group_step": 20}
E_ARG, E_HIP, E_STATE = -1, -2, -3
M20, M24 = 1 << 20, 1 << 24
GOOD = (2, 7, 0, 4, 3, 3)
BAD = [((-1, 0, 0, 4, 0, 0), "pad"), ((M20 + 1, 0, 0, 4, 0, 0), "pad"), ((0, -1, 0, 4, 0, 0), "max_len"), ((0, M24 + 1, 0, 4, 0, 0), "max_len"),
       ((0, 0, -1, 4, 0, 0), "min_len"), ((0, 7, 1, 4, 0, 0), "min_len"), ((0, 0, 3, 4, 0, 0), "min_len"), ((0, 0, 0, 0, 0, 0), "hop"),
       ((0, 0, 0, 4, -1, 0), "lead"), ((0, 0, 0, 4, 0, -1), "tail")]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _configure(lib, built, ctx, first=(0, 2, 5, 7), members=(0, 2, 2, 3, 6, 4, 5)):
    f, m = np.asarray(first, np.int32), np.asarray(members, np.int32)
    return lib.uvad_fuse_configure(ctx, C.byref(built.FuseCfg(0, 0.5, 0.5)), f.ctypes.data, m.ctypes.data, None, len(first) - 1)


def test_entries_in_header_binding_and_export_list(built):
    text = open(os.path.join(ROOT, "include", "uvad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]) == nargs, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_gate_group_history"][0] is C.c_int64 and built.SIGNATURES["uvad_gate_group_max_out"][0] is C.c_int64
    assert built.SIGNATURES["uvad_gate_group_best_history"][0] is C.c_int and built.SIGNATURES["uvad_gate_group_state_bytes"][0] is C.c_size_t
    assert re.search(r"#define UVAD_GATE_UNSYNC\s+16\b", src) and built.GATE_UNSYNC == gg.UNSYNC == 16
    assert re.search(r"#define UVAD_GATE_CHANNEL\(flags\) \(\(\(flags\) >> 8\) & 0xff\)", src) and gg.channel(0x1234) == 0x12
    assert built.load().uvad_abi_version() == built.ABI_VERSION == 5                # appended: the number stays
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bgate_group\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "gate_group.hip")).read()
    assert "launch_state_reset(state, header_words(h)" in kernel and "gate_group_step_kernel" in kernel   # the reset is state_reset.hip's
    assert "asm" not in kernel and "atomic" not in re.sub(r"//.*", "", kernel)      # no inline assembly; no atomics in the code
    assert "__ballot" in kernel and "__popcll" in kernel
    assert kernel.count("hipLaunchKernelGGL(gate_group_step_kernel") == 2           # one launch per step: the int16 or the f32 form
    for cite in ("uvad_fuse_pick", "uvad_cuts_gather", "uvad_gate_step"):           # what the entry points stand in for
        assert cite in re.search(r"Live speech gate for fused groups.*?\*/", text, re.S).group(0)


def test_size_helpers_against_their_formulas(built):
    lib = built.load()
    cfg = lambda q: C.byref(built.CutsCfg(*q))
    for q in (GOOD, (0, 0, 0, 4, 0, 0), (5, 1, 0, 160, 120, 120), (0, 1000, 0, 270, 0, 721), (M20, 1, 0, 3, 1, 2)):
        for lag in (0, 1, 10, 500):
            for chunk in (1, 6, 320, 321):
                for D in (1, 3, 25, 1000, M24):
                    assert lib.uvad_gate_group_history(cfg(q), lag, chunk, D) == gg.history(q, lag, chunk, D)
                    assert lib.uvad_gate_group_best_history(cfg(q), lag, chunk, D) == gg.best_history(q, lag, chunk, D)
                assert lib.uvad_gate_group_history(cfg(q), lag, chunk, 1) == lib.uvad_gate_history(cfg(q), lag, chunk)   # D = 1: the mono gate's
        for ld in (0, 1, 8, 39):
            for D in (1, 25, M24):
                assert lib.uvad_gate_group_max_out(cfg(q), ld, 320, D) == gg.max_out(q, ld, 320, D) == \
                    lib.uvad_gate_max_out(cfg(q), ld, 320, 1 << 20) + D * q[3]
    g = cfg(GOOD)
    for fn in (lib.uvad_gate_group_history, lib.uvad_gate_group_best_history):
        assert fn(None, 3, 320, 5) == -1
        for args in ((-1, 320, 5), (3, 0, 5), (3, M24 + 1, 5), (3, 320, 0), (3, 320, -1), (3, 320, M24 + 1)):
            assert fn(g, *args) == -1, args
        for q, _ in BAD:
            assert fn(cfg(q), 3, 320, 5) == -1, q
    assert lib.uvad_gate_group_best_history(cfg((0, 0, 0, 1, 0, 0)), (1 << 31) - 1, M24, M24) == -1                      # past int32
    assert lib.uvad_gate_group_max_out(None, 8, 320, 5) == -1
    for args in ((-1, 320, 5), (8, 0, 5), (8, M24 + 1, 5), (8, 320, 0), (8, 320, M24 + 1)):
        assert lib.uvad_gate_group_max_out(g, *args) == -1, args
    for q, _ in BAD:
        assert lib.uvad_gate_group_max_out(cfg(q), 8, 320, 5) == -1, q
    assert lib.uvad_gate_group_max_out(cfg((M20, 1, 0, (1 << 31) - 1, 0, 0)), (1 << 31) - 1, 1, M24) == (1 << 63) - 1     # saturates


def test_state_before_configure_then_sizes_and_refusals(built):
    """Each call below is refused on its arguments alone, so it reads the same without a GPU (where the configuration's upload has failed)
    and with one.  The pointers are never dereferenced."""
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)
    good = built.CutsCfg(*GOOD)
    try:
        size = lambda q=GOOD, unit=2, hist=640, bh=40: lib.uvad_gate_group_state_bytes(ctx, C.byref(built.CutsCfg(*q)), unit, hist, bh)

        def reset(state=fake, nbytes=1 << 40, q=C.byref(good), unit=2, hist=640, bh=40, D=5):
            return lib.uvad_gate_group_reset(ctx, state, nbytes, q, unit, hist, bh, D, None)

        def step(chunk_p=fake, chunk=320, B=7, best=fake, ld_best=8, best_counts=fake, labels=fake, ld_lab=8, lab_counts=fake, state=fake,
                 nbytes=1 << 40, out=fake, ld_out=64, seg=fake, max_seg=4, seg_counts=fake):
            return lib.uvad_gate_group_step(ctx, chunk_p, chunk, B, best, ld_best, best_counts, labels, ld_lab, lab_counts, None, None, state, nbytes,
                                            out, ld_out, seg, max_seg, seg_counts, None)

        # before uvad_fuse_configure: no size, and every call is a state error that names the missing call
        assert size() == 0
        assert reset() == E_STATE and "uvad_fuse_configure" in err()
        assert step() == E_STATE and "uvad_fuse_configure" in err()
        code = _configure(lib, built, ctx)            # three groups, N = 7 member slots over rows 0 .. 6, row 2 in two of them
        assert code in (0, E_HIP)
        # the size: a header, 96 bytes and a best ring per group, a PCM ring per member slot, rings rounded up to 16 bytes
        for unit in (2, 4):
            for hist, bh in ((640, 40), (641, 41), (8, 1), (1000, 16), (1001, 17)):
                assert size(unit=unit, hist=hist, bh=bh) == gg.state_bytes(3, 7, unit, hist, bh), (unit, hist, bh)
        assert size((0, 0, 0, 1, 0, 0)) == size()                                   # it does not depend on the cut parameters
        for q, _ in BAD:
            assert size(q) == 0, q
        for kw in ({"unit": 1}, {"unit": 3}, {"unit": 8}, {"hist": 0}, {"hist": 1 << 31}, {"bh": 0}, {"bh": -3}):
            assert size(**kw) == 0, kw
        assert lib.uvad_gate_group_state_bytes(ctx, None, 2, 640, 40) == 0
        assert lib.uvad_gate_group_state_bytes(None, C.byref(good), 2, 640, 40) == 0
        need = size()
        # reset
        for q, word in BAD:
            assert reset(q=C.byref(built.CutsCfg(*q))) == E_ARG and word in err(), q
        for kw, word in (({"q": None}, "cfg"), ({"unit": 3}, "unit_bytes"), ({"unit": 8}, "unit_bytes"), ({"hist": 0}, "history"),
                         ({"hist": 1 << 31}, "history"), ({"bh": 0}, "best_history"), ({"bh": -1}, "best_history"), ({"D": 0}, "decide_frames"),
                         ({"D": -4}, "decide_frames"), ({"D": M24 + 1}, "decide_frames"), ({"state": None}, "d_state"),
                         ({"nbytes": need - 1}, f"need {need} bytes"), ({"nbytes": 0}, f"need {need} bytes")):
            assert reset(**kw) == E_ARG and word in err(), kw
        assert lib.uvad_gate_group_reset(None, fake, need, C.byref(good), 2, 640, 40, 5, None) == E_ARG
        # step
        for kw, word in (({"B": 6}, "largest configured member index (6)"), ({"B": 0}, "B"), ({"chunk": 0}, "chunk"), ({"chunk": M24 + 1}, "chunk"),
                         ({"ld_lab": -1}, "ld_lab"), ({"ld_best": -1}, "ld_best"), ({"ld_out": -1}, "ld_out"), ({"max_seg": -1}, "max_seg"),
                         ({"chunk_p": None}, "d_chunk"), ({"state": None}, "d_state"), ({"seg_counts": None}, "d_seg_counts"),
                         ({"labels": None}, "d_labels"), ({"lab_counts": None}, "d_lab_counts"), ({"best": None}, "d_best"),
                         ({"best_counts": None}, "d_best_counts"), ({"out": None}, "d_out"), ({"seg": None}, "d_seg")):
            assert step(**kw) == E_ARG and word in err(), kw
        assert step() == E_STATE and "uvad_gate_group_reset" in err()               # arguments in order, but the state was never reset
        assert step(labels=None, lab_counts=None, ld_lab=0, best=None, best_counts=None, ld_best=0) == E_STATE   # NULL goes with a zero width
        assert step(out=None, ld_out=0, seg=None, max_seg=0) == E_STATE             # no outputs but the counts
        assert lib.uvad_gate_group_step(None, fake, 320, 7, fake, 8, fake, fake, 8, fake, None, None, fake, need, fake, 64, fake, 4, fake, None) == E_ARG
        if code == E_HIP:                             # no device: a reset whose arguments are accepted stops at "not on the device"
            assert reset(nbytes=need) == E_HIP and "not on the device" in err()
    finally:
        lib.uvad_destroy(ctx)


def test_group_gate_keyword_of_the_pools(built):
    from uvad_amd.postprocess import group_gate_config
    from uvad_amd.runtime import VadRuntime
    for opener in (VadRuntime.window_slots_open, VadRuntime.wav_window_slots_open):
        assert inspect.signature(opener).parameters["group_gate"].default is None
        # refused before anything is allocated: the runtime (self) is never touched
        for kw in (dict(), dict(fuse={"groups": [[0, 1]]}), dict(endpoint={"onset": 0.5})):
            with pytest.raises(ValueError, match="group_gate needs fuse= and endpoint="):
                opener(None, 4, 320, group_gate={"decide_frames": 3}, **kw)
        for bad in ({}, {"decide_frames": 0}, {"decide_frames": M24 + 1}, {"decide_frames": 2.5}, {"decide_frames": True},
                    {"decide_frames": 3, "min_len": 1}, {"decide_frames": 3, "window": 4}, 3):
            with pytest.raises(ValueError, match="group_gate|decide_frames"):
                opener(None, 4, 320, group_gate=bad, fuse={"groups": [[0, 1]]}, endpoint={"onset": 0.5})
    assert group_gate_config({"decide_frames": 25, "max_len": 1000, "pad": None}, {}, {}) == {"decide_frames": 25, "max_len": 1000}
    # the mono gate behind a fused pool stays refused, with its message
    with pytest.raises(ValueError, match="gate= together with fuse= is not built: the gate would need a channel choice per fragment"):
        VadRuntime._slots_fuse(None, {"B": 4, "out": None}, {"groups": [[0, 1], [2, 3]]}, {})
    assert list(inspect.signature(VadRuntime._slots_fuse).parameters) == ["self", "st", "fuse", "gate"]
