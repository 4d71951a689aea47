"""CPU checks of the live endpointer's entry points (uvad_endpoint_*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; the configuration struct's size; uvad_endpoint_state_bytes is 0 for every bad configuration and grows with B; and the refusals
that are made before the library touches a device."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_endpoint_state_bytes", "uvad_endpoint_reset", "uvad_endpoint_step"]
E_ARG, E_STATE = -1, -3


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_endpoint_entries_in_header_binding_and_export_list(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_endpoint_state_bytes"][0] is C.c_size_t
    assert built.SIGNATURES["uvad_endpoint_reset"][0] is C.c_int and len(built.SIGNATURES["uvad_endpoint_reset"][1]) == 6
    assert built.SIGNATURES["uvad_endpoint_step"][0] is C.c_int and len(built.SIGNATURES["uvad_endpoint_step"][1]) == 16
    assert built.load().uvad_abi_version() == built.ABI_VERSION          # header and binding carry one number
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bendpoint\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "endpoint.hip")).read()
    assert "launch_state_reset(state, header_words(h)" in kernel and "endpoint_step_kernel" in kernel and "asm" not in kernel


def test_cfg_struct_matches_the_header(built):
    src = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} uvad_endpoint_cfg;", src).group(1)
    fields = re.findall(r"\b(int|float)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [("int", "kernel"), ("int", "pad"), ("float", "threshold")]
    assert [f[0] for f in built.EndpointCfg._fields_] == ["kernel", "pad", "threshold"]
    assert C.sizeof(built.EndpointCfg) == 12
    assert (built.SLOT_START, built.SLOT_END) == (1, 2)


def test_state_bytes_is_zero_on_a_bad_configuration_and_grows_with_B(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    try:
        size = lambda B, k, p, t: lib.uvad_endpoint_state_bytes(ctx, B, C.byref(built.EndpointCfg(k, p, t)))
        sizes = [size(B, 25, 10, 0.5) for B in (1, 2, 5, 512, 4096)]
        assert all(v > 0 for v in sizes) and sizes == sorted(set(sizes))
        assert (sizes[3] - sizes[2]) % (512 - 5) == 0 and (sizes[3] - sizes[2]) // (512 - 5) <= 64       # a few dozen bytes per feed
        for k, p, t in ((1, 0, 0.5), (255, 1 << 20, 0.3), (3, 7, -1.0), (49, 0, 1e30)):
            assert size(5, k, p, t) == sizes[2], (k, p, t)                                                # the size does not depend on them
        for k, p, t in ((0, 0, 0.5), (-1, 0, 0.5), (2, 0, 0.5), (24, 0, 0.5), (256, 0, 0.5), (257, 0, 0.5),
                        (25, -1, 0.5), (25, (1 << 20) + 1, 0.5), (25, 0, math.nan), (25, 0, math.inf), (25, 0, -math.inf)):
            assert size(5, k, p, t) == 0, (k, p, t)
        assert size(0, 25, 0, 0.5) == 0 and size(-3, 25, 0, 0.5) == 0
        assert lib.uvad_endpoint_state_bytes(ctx, 5, None) == 0
        assert lib.uvad_endpoint_state_bytes(None, 5, C.byref(built.EndpointCfg(25, 0, 0.5))) == 0
    finally:
        lib.uvad_destroy(ctx)


def test_refusals_made_before_a_device_is_touched(built):
    """Each call below is refused on its arguments alone, so it reads the same without a GPU (where uvad_create has failed but returned
    its context) and with one."""
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)          # never dereferenced
    good = built.EndpointCfg(25, 10, 0.5)
    need = lib.uvad_endpoint_state_bytes(ctx, 4, C.byref(good))
    try:
        for cfg, word in ((built.EndpointCfg(24, 0, 0.5), "kernel"), (built.EndpointCfg(257, 0, 0.5), "kernel"), (built.EndpointCfg(0, 0, 0.5), "kernel"),
                          (built.EndpointCfg(25, -1, 0.5), "pad"), (built.EndpointCfg(25, (1 << 20) + 1, 0.5), "pad"),
                          (built.EndpointCfg(25, 0, math.nan), "threshold"), (built.EndpointCfg(25, 0, math.inf), "threshold")):
            assert lib.uvad_endpoint_reset(ctx, fake, need, 4, C.byref(cfg), None) == E_ARG and word in err()
        assert lib.uvad_endpoint_reset(ctx, fake, need, 0, C.byref(good), None) == E_ARG
        assert lib.uvad_endpoint_reset(ctx, None, need, 4, C.byref(good), None) == E_ARG
        assert lib.uvad_endpoint_reset(ctx, fake, need, 4, None, None) == E_ARG
        assert lib.uvad_endpoint_reset(ctx, fake, need - 1, 4, C.byref(good), None) == E_ARG and f"need {need} bytes" in err()
        step = lambda probs=fake, ld_in=8, counts=fake, B=4, state=fake, nbytes=need, events=fake, max_events=4, ev_counts=fake, labels=None, ld_lab=0, \
            lab_counts=None: lib.uvad_endpoint_step(ctx, probs, ld_in, counts, None, B, state, nbytes, events, max_events, ev_counts, None, labels,
                                                    ld_lab, lab_counts, None)
        for kw in ({"probs": None}, {"counts": None}, {"ev_counts": None}, {"state": None}, {"B": 0}, {"ld_in": 0}, {"events": None},
                   {"max_events": -1}, {"labels": fake, "ld_lab": 64}):
            assert step(**kw) == E_ARG, kw
        assert step() == E_STATE and "uvad_endpoint_reset" in err()           # arguments in order, but the state was never reset
        assert step(events=None, max_events=0) == E_STATE
    finally:
        lib.uvad_destroy(ctx)
