"""CPU checks of the live speech gate's entry points (uvad_gate_*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; uvad_gate_state_bytes is 0 for every bad configuration and grows linearly in B and in the ring's length; the helper bounds
against their formulas (tests/gate_ref.py) and monotone; and every refusal that is made before the library touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import gate_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_gate_state_bytes", "uvad_gate_history", "uvad_gate_max_out", "uvad_gate_max_seg", "uvad_gate_reset", "uvad_gate_step"]
E_ARG, E_STATE = -1, -3
M = 1 << 20
GOOD = (2, 7, 0, 4, 3, 3)
BAD = [((-1, 0, 0, 4, 0, 0), "pad"), ((M + 1, 0, 0, 4, 0, 0), "pad"), ((0, -1, 0, 4, 0, 0), "max_len"), ((0, (1 << 24) + 1, 0, 4, 0, 0), "max_len"),
       ((0, 0, -1, 4, 0, 0), "min_len"), ((0, 7, 7, 4, 0, 0), "min_len"), ((0, 7, 1, 4, 0, 0), "min_len"), ((0, 0, 3, 4, 0, 0), "min_len"),
       ((0, 0, 0, 0, 0, 0), "hop"), ((0, 0, 0, 4, -1, 0), "lead"), ((0, 0, 0, 4, 0, -1), "tail")]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_entries_in_header_binding_and_export_list(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_gate_history"] == (C.c_int64, [C.POINTER(built.CutsCfg), C.c_int, C.c_int])
    assert built.SIGNATURES["uvad_gate_max_out"][0] is C.c_int64 and built.SIGNATURES["uvad_gate_state_bytes"][0] is C.c_size_t
    assert len(built.SIGNATURES["uvad_gate_step"][1]) == 16 and len(built.SIGNATURES["uvad_gate_reset"][1]) == 8
    assert C.sizeof(built.GateSeg) == 32 and built.GateSeg.offset.offset == 16 and built.GateSeg.n_stored.offset == 28
    assert [f[0] for f in built.GateSeg._fields_] == list(gr.SEG_DTYPE.names)
    assert (built.GATE_FIRST, built.GATE_LAST, built.GATE_LOST, built.GATE_SHORT) == (1, 2, 4, 8)
    for word, value in (("FIRST", 1), ("LAST", 2), ("LOST", 4), ("SHORT", 8)):
        assert re.search(rf"#define UVAD_GATE_{word}\s+{value}\b", src)
    assert re.search(r"#define UVAD_ABI_VERSION 5\b", src)
    assert built.ABI_VERSION == 5 and built.load().uvad_abi_version() == 5         # appended: the number stays
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bgate\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "gate.hip")).read()
    assert "launch_state_reset(state, header_words(h)" in kernel and "gate_step_kernel" in kernel         # the reset is state_reset.hip's
    assert "asm" not in kernel and "atomic" not in kernel.lower().replace("no atomics", "")
    assert kernel.count("hipLaunchKernelGGL(gate_step_kernel") == 2                 # one launch per step: the int16 or the f32 form


def test_state_bytes(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    try:
        size = lambda B, unit, hist, q=GOOD: lib.uvad_gate_state_bytes(ctx, B, C.byref(built.CutsCfg(*q)), unit, hist)
        for unit in (2, 4):
            per = 16 // unit                                                        # rings are rounded up to 16 bytes
            sizes = [size(B, unit, 80 * per) for B in (1, 2, 5, 512)]
            assert all(v > 0 for v in sizes) and sizes[1] - sizes[0] == (sizes[2] - sizes[1]) // 3 == (sizes[3] - sizes[2]) // 507
            assert sizes[1] - sizes[0] >= 80 * per * unit                           # a slot holds its ring
            by_h = [size(5, unit, h * per) for h in (1, 2, 10, 1000)]
            assert by_h[1] - by_h[0] == 5 * 16 and by_h[2] - by_h[1] == 8 * 5 * 16 and by_h[3] - by_h[2] == 990 * 5 * 16
            assert size(5, unit, 80 * per - 1) == size(5, unit, 80 * per) and size(5, unit, 80 * per + 1) > size(5, unit, 80 * per)
        for q in ((0, 0, 0, 1, 0, 0), (M, 1 << 24, 0, 270, 0, 721), (5, 1, 0, 160, 120, 120)):
            assert size(5, 2, 640, q) == size(5, 2, 640)                            # the size does not depend on the cut parameters
        for q, _ in BAD:
            assert size(5, 2, 640, q) == 0, q
        for B, unit, hist in ((0, 2, 640), (-1, 2, 640), (5, 1, 640), (5, 3, 640), (5, 8, 640), (5, 0, 640), (5, 2, 0), (5, 2, -7), (5, 2, 1 << 31)):
            assert size(B, unit, hist) == 0, (B, unit, hist)
        assert size(1, 4, (1 << 31) - 1) > 4 * ((1 << 31) - 1)
        assert lib.uvad_gate_state_bytes(ctx, 5, None, 2, 640) == 0
        assert lib.uvad_gate_state_bytes(None, 5, C.byref(built.CutsCfg(*GOOD)), 2, 640) == 0
    finally:
        lib.uvad_destroy(ctx)


def test_helper_bounds_against_their_formulas_and_monotone(built):
    lib = built.load()
    cfg = lambda q: C.byref(built.CutsCfg(*q))
    qs = [GOOD, (0, 0, 0, 4, 0, 0), (5, 1, 0, 160, 120, 120), (0, 7, 0, 270, 0, 721), (M, 1, 0, 3, 1, 2), (9, 1 << 24, 0, 1, 0, 0)]
    for q in qs:
        hist = [lib.uvad_gate_history(cfg(q), lag, chunk) for lag in (0, 1, 10, 500) for chunk in (1, 320)]
        assert hist == [gr.history(q, lag, chunk) for lag in (0, 1, 10, 500) for chunk in (1, 320)]
        assert all(lib.uvad_gate_history(cfg(q), lag + 1, 64) > lib.uvad_gate_history(cfg(q), lag, 64) for lag in (0, 3, 99))
        assert all(lib.uvad_gate_history(cfg(q), 4, c + 1) > lib.uvad_gate_history(cfg(q), 4, c) for c in (1, 63, 320))
        segs = [lib.uvad_gate_max_seg(cfg(q), ld) for ld in range(0, 40)] + [lib.uvad_gate_max_seg(cfg(q), 1 << 18)]
        assert segs == [gr.max_seg(q, ld) for ld in range(0, 40)] + [gr.max_seg(q, 1 << 18)]
        assert segs == sorted(segs) and segs[0] >= 3
        outs = [lib.uvad_gate_max_out(cfg(q), ld, 320, 1 << 20) for ld in range(0, 40)]
        assert outs == [gr.max_out(q, ld, 320) for ld in range(0, 40)] and outs == sorted(outs)
        assert lib.uvad_gate_max_out(cfg(q), 8, 321, 1 << 20) > lib.uvad_gate_max_out(cfg(q), 8, 320, 1 << 20)
        assert lib.uvad_gate_max_out(cfg(q), 8, 320, 320) == lib.uvad_gate_max_out(cfg(q), 8, 320, 1 << 20)     # lost samples are written too
    assert lib.uvad_gate_max_seg(cfg((M, 1, 0, 4, 0, 0)), (1 << 31) - 1) == (1 << 31) - 1                      # saturates
    assert lib.uvad_gate_max_out(cfg((M, 1, 0, (1 << 31) - 1, 0, 0)), (1 << 31) - 1, 1, 1) == (1 << 63) - 1
    for q, _ in BAD:
        assert lib.uvad_gate_history(cfg(q), 3, 320) == -1 and lib.uvad_gate_max_seg(cfg(q), 8) == -1, q
        assert lib.uvad_gate_max_out(cfg(q), 8, 320, 640) == -1, q
    assert lib.uvad_gate_history(None, 3, 320) == -1 and lib.uvad_gate_max_seg(None, 8) == -1 and lib.uvad_gate_max_out(None, 8, 320, 640) == -1
    g = cfg(GOOD)
    assert lib.uvad_gate_history(g, -1, 320) == -1 and lib.uvad_gate_history(g, 3, 0) == -1 and lib.uvad_gate_history(g, 3, (1 << 24) + 1) == -1
    assert lib.uvad_gate_max_seg(g, -1) == -1
    assert lib.uvad_gate_max_out(g, -1, 320, 640) == -1 and lib.uvad_gate_max_out(g, 8, 0, 640) == -1
    assert lib.uvad_gate_max_out(g, 8, 320, 319) == -1 and lib.uvad_gate_max_out(g, 8, 320, 1 << 31) == -1       # history < chunk, > 2^31 - 1
    assert lib.uvad_gate_max_out(g, 8, 320, 320) > 0


def test_refusals_made_before_a_device_is_touched(built):
    """Each call below is refused on its arguments alone, so it reads the same without a GPU (where uvad_create has failed but returned
    its context) and with one.  The pointers are never dereferenced: the outputs cannot have been touched.  (history < chunk is a step's
    refusal against the reset's history: it needs a reset state, and is checked on the GPU.)"""
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)
    good = built.CutsCfg(*GOOD)
    need = lib.uvad_gate_state_bytes(ctx, 4, C.byref(good), 2, 640)
    try:
        reset = lambda state=fake, nbytes=need, B=4, q=C.byref(good), unit=2, hist=640: lib.uvad_gate_reset(ctx, state, nbytes, B, q, unit, hist, None)
        for q, word in BAD:
            assert reset(q=C.byref(built.CutsCfg(*q))) == E_ARG and word in err(), q
        for kw, word in (({"q": None}, "cfg"), ({"B": 0}, "B"), ({"unit": 3}, "unit_bytes"), ({"unit": 8}, "unit_bytes"), ({"hist": 0}, "history"),
                         ({"hist": 1 << 31}, "history"), ({"state": None}, "d_state"), ({"nbytes": need - 1}, f"need {need} bytes")):
            assert reset(**kw) == E_ARG and word in err(), kw

        def step(chunk_p=fake, chunk=320, labels=fake, ld_lab=8, lab_counts=fake, B=4, state=fake, nbytes=need, out=fake, ld_out=64, seg=fake, max_seg=4,
                 seg_counts=fake):
            return lib.uvad_gate_step(ctx, chunk_p, chunk, labels, ld_lab, lab_counts, None, B, state, nbytes, out, ld_out, seg, max_seg, seg_counts, None)

        for kw, word in (({"B": 0}, "B"), ({"chunk": 0}, "chunk"), ({"chunk": (1 << 24) + 1}, "chunk"), ({"ld_lab": -1}, "ld_lab"),
                         ({"ld_out": -1}, "ld_out"), ({"max_seg": -1}, "max_seg"), ({"chunk_p": None}, "d_chunk"), ({"state": None}, "d_state"),
                         ({"seg_counts": None}, "d_seg_counts"), ({"labels": None}, "d_labels"), ({"lab_counts": None}, "d_lab_counts"),
                         ({"out": None}, "d_out"), ({"seg": None}, "d_seg")):
            assert step(**kw) == E_ARG and word in err(), kw
        assert step() == E_STATE and "uvad_gate_reset" in err()                     # arguments in order, but the state was never reset
        assert step(labels=None, lab_counts=None, ld_lab=0) == E_STATE              # no labels with ld_lab = 0
        assert step(out=None, ld_out=0, seg=None, max_seg=0) == E_STATE             # no outputs but the counts
    finally:
        lib.uvad_destroy(ctx)
