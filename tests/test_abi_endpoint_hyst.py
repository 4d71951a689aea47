"""CPU checks of the live hysteresis endpointer's entry points (uvad_endpoint_hyst_*, include/uvad.h): declared in the header, bound in the
ctypes table and exported; uvad_endpoint_hyst_state_bytes is 0 for every bad configuration, grows with B by at most 64 bytes per feed and
does not depend on the configuration's values; uvad_endpoint_hyst_lag against its formula; and the refusals that are made before the
library touches a device."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_endpoint_hyst_lag", "uvad_endpoint_hyst_state_bytes", "uvad_endpoint_hyst_reset", "uvad_endpoint_hyst_step"]
E_ARG, E_STATE = -1, -3
M = 1 << 20
BAD = [((math.nan, 0.3, 0, 0, 0, 0), "onset"), ((math.inf, 0.3, 0, 0, 0, 0), "onset"), ((0.7, math.nan, 0, 0, 0, 0), "offset"),
       ((0.7, -math.inf, 0, 0, 0, 0), "offset"), ((0.3, 0.7, 0, 0, 0, 0), "offset"), ((0.7, 0.3, -1, 0, 0, 0), "min_on"),
       ((0.7, 0.3, M + 1, 0, 0, 0), "min_on"), ((0.7, 0.3, 0, -1, 0, 0), "min_off"), ((0.7, 0.3, 0, M + 1, 0, 0), "min_off"),
       ((0.7, 0.3, 0, 0, -1, 0), "pad_on"), ((0.7, 0.3, 0, 0, M + 1, 0), "pad_on"), ((0.7, 0.3, 0, 0, 0, -1), "pad_off"),
       ((0.7, 0.3, 0, 0, 0, M + 1), "pad_off")]


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
    assert built.SIGNATURES["uvad_endpoint_hyst_lag"] == (C.c_int, [C.POINTER(built.BinarizeCfg)])
    assert built.SIGNATURES["uvad_endpoint_hyst_state_bytes"][0] is C.c_size_t
    assert built.SIGNATURES["uvad_endpoint_hyst_reset"][0] is C.c_int and len(built.SIGNATURES["uvad_endpoint_hyst_reset"][1]) == 6
    # the step's argument list is uvad_endpoint_step's: a slot pool's buffers serve both
    assert built.SIGNATURES["uvad_endpoint_hyst_step"] == built.SIGNATURES["uvad_endpoint_step"]
    assert built.ABI_VERSION == 5 and built.load().uvad_abi_version() == 5         # appended: the number stays
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bendpoint_hyst\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "endpoint_hyst.hip")).read()
    assert "launch_state_reset(state, header_words(h)" in kernel and "endpoint_hyst_step_kernel" in kernel
    assert "asm" not in kernel and "atomic" not in kernel.replace("no atomics", "") and "__shared__" not in kernel


def test_state_bytes(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    try:
        size = lambda B, *q: lib.uvad_endpoint_hyst_state_bytes(ctx, B, C.byref(built.BinarizeCfg(*q)))
        sizes = [size(B, 0.7, 0.3, 25, 10, 3, 6) for B in (1, 2, 5, 512, 4096)]
        assert all(v > 0 for v in sizes) and sizes == sorted(set(sizes))
        assert (sizes[3] - sizes[2]) % (512 - 5) == 0 and (sizes[3] - sizes[2]) // (512 - 5) <= 64       # at most 64 bytes per feed
        assert (sizes[4] - sizes[3]) // (4096 - 512) == (sizes[1] - sizes[0])
        for q in ((0.5, 0.5, 0, 0, 0, 0), (1e30, -1e30, M, M, M, M), (0.3, 0.3, 0, 1, 7, 7), (-1.0, -2.0, 300, 0, 40, 0)):
            assert size(5, *q) == sizes[2], q                                                             # the size does not depend on them
        for q, _ in BAD:
            assert size(5, *q) == 0, q
        assert size(0, 0.7, 0.3, 0, 0, 0, 0) == 0 and size(-3, 0.7, 0.3, 0, 0, 0, 0) == 0
        assert lib.uvad_endpoint_hyst_state_bytes(ctx, 5, None) == 0
        assert lib.uvad_endpoint_hyst_state_bytes(None, 5, C.byref(built.BinarizeCfg(0.7, 0.3, 0, 0, 0, 0))) == 0
    finally:
        lib.uvad_destroy(ctx)


def test_lag_is_min_on_plus_D(built):
    lib = built.load()
    lag = lambda *q: lib.uvad_endpoint_hyst_lag(C.byref(built.BinarizeCfg(*q)))
    for min_on in (0, 1, 25, M):
        for min_off in (0, 1, 2, 10, M):
            for pad_on, pad_off in ((0, 0), (3, 0), (0, 6), (3, 6), (M, M)):
                assert lag(0.7, 0.3, min_on, min_off, pad_on, pad_off) == min_on + pad_on + pad_off + max(min_off - 1, 0)
    assert lag(0.5, 0.5, 0, 0, 0, 0) == 0 and lag(0.5, 0.5, 0, 1, 0, 0) == 0 and lag(0.5, 0.5, 0, 2, 0, 0) == 1
    for q, _ in BAD:
        assert lag(*q) == -1, q
    assert lib.uvad_endpoint_hyst_lag(None) == -1


def test_refusals_made_before_a_device_is_touched(built):
    """Each call below is refused on its arguments alone, so it reads the same without a GPU (where uvad_create has failed but returned
    its context) and with one.  The pointers are never dereferenced: the outputs cannot have been touched."""
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)
    good = built.BinarizeCfg(0.7, 0.3, 3, 4, 2, 5)
    need = lib.uvad_endpoint_hyst_state_bytes(ctx, 4, C.byref(good))
    try:
        for q, word in BAD:
            assert lib.uvad_endpoint_hyst_reset(ctx, fake, need, 4, C.byref(built.BinarizeCfg(*q)), None) == E_ARG and word in err(), q
        assert lib.uvad_endpoint_hyst_reset(ctx, fake, need, 4, None, None) == E_ARG and "cfg" in err()
        assert lib.uvad_endpoint_hyst_reset(ctx, fake, need, 0, C.byref(good), None) == E_ARG
        assert lib.uvad_endpoint_hyst_reset(ctx, None, need, 4, C.byref(good), None) == E_ARG
        assert lib.uvad_endpoint_hyst_reset(ctx, fake, need - 1, 4, C.byref(good), None) == E_ARG and f"need {need} bytes" in err()
        step = lambda probs=fake, ld_in=8, counts=fake, B=4, state=fake, nbytes=need, events=fake, max_events=4, ev_counts=fake, labels=None, ld_lab=0, \
            lab_counts=None: lib.uvad_endpoint_hyst_step(ctx, probs, ld_in, counts, None, B, state, nbytes, events, max_events, ev_counts, None,
                                                         labels, ld_lab, lab_counts, None)
        for kw in ({"probs": None}, {"counts": None}, {"ev_counts": None}, {"state": None}, {"B": 0}, {"ld_in": 0}, {"ld_in": (1 << 18) + 1},
                   {"events": None}, {"max_events": -1}, {"labels": fake, "ld_lab": 64}):
            assert step(**kw) == E_ARG, kw
        assert step() == E_STATE and "uvad_endpoint_hyst_reset" in err()      # arguments in order, but the state was never reset
        assert step(events=None, max_events=0) == E_STATE
    finally:
        lib.uvad_destroy(ctx)
