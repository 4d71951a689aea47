"""Checks of the reverberation entry points (uvad_reverb_*, include/uvad.h) that need no GPU: declared, bound and exported; the struct
layout; the header's statement of the counter, the threshold, the delay, z, g and the plan words; the size helpers; the refusals made
before the library touches a device (fake pointers that are never dereferenced)."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_reverb_state_bytes", "uvad_reverb_ws_bytes", "uvad_reverb_reset", "uvad_reverb_step", "uvad_reverb_apply"]
E_ARG, E_STATE = -1, -3


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_entries_in_header_binding_and_export_list(built):
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert name in built.SIGNATURES and len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", raw) and built.ABI_VERSION == 5 and built.load().uvad_abi_version() == 5
    step, apply = built.SIGNATURES["uvad_reverb_step"][1], built.SIGNATURES["uvad_reverb_apply"][1]
    assert step[4] is C.c_int64 and apply[8] is C.c_int64 and apply[9] is C.c_uint64 and apply[:8] == step[:8] and apply[10:] == step[8:]
    assert step == built.SIGNATURES["uvad_mix_step"][1] and apply == built.SIGNATURES["uvad_mix_apply"][1]      # the mix block's argument order
    assert src.index("uvad_mix_apply(") < src.index("uvad_reverb_state_bytes(") < src.index("uvad_set_gemm_mode(")   # appended behind the mix block


def test_struct_layout_and_constants(built):
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} uvad_reverb_cfg;", raw).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in built.ReverbCfg._fields_] == ["prob", "normalize", "align", "max_taps", "seed"]
    R = built.ReverbCfg
    assert C.sizeof(R) == 24 and (R.prob.offset, R.normalize.offset, R.align.offset, R.max_taps.offset, R.seed.offset) == (0, 4, 8, 12, 16)
    for name, val in (("UVAD_REVERB_PLAN_WORDS", built.REVERB_PLAN_WORDS), ("UVAD_REVERB_MAX_TAPS", built.REVERB_MAX_TAPS),
                      ("UVAD_REVERB_TILE", built.REVERB_TILE), ("UVAD_REVERB_K_CHUNK", built.REVERB_K_CHUNK)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", raw).group(1)) == val, name
    assert built.REVERB_MAX_TAPS >= 32768                           # responses of 2.048 s and more are served


def test_header_states_the_draws_the_sum_and_the_plan():
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    block = raw[raw.index("Reverberation of training batches"):raw.index("} uvad_reverb_cfg;")]
    for cite in ("Philox4x32-10", "(row0 + b, 0x52560000, draw_lo, draw_hi)", "(seed_lo,", "(uint64)w0 < floor(prob 2^32)", "r = (w1 n_rirs) >> 32",
                 "words 2 and 3 are reserved", "the smallest k < K_r at which |h_r[k]| is largest", "A NaN never wins",
                 "min(length, max_taps)", "z[i] = sum_{k = 0}^{K_r - 1} h_r[k] x[i + d - k]", "d = delay_r when align != 0 and d = 0 otherwise",
                 "is 0 and is never read", "f32-exact", "function of (K_r, i) alone", "No atomics", "g = (float)sqrt(E_in / E_out)",
                 "g = 1.0f when either energy is 0", "out = fl32(z g)", "no fused operation", "the input's f32 value bit for bit", "q / 32768",
                 "are +0 in d_out", "byte 56", "{applied (0 / 1), r, d, the bits of g}", "{0, 0, 0, the bits of 1.0f}", "d_out == d_in is refused",
                 "UNPINNED", "does not depend on the bank's size", "UVAD_E_STATE: a state that was never reset"):
        assert cite in block, cite
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    kernel = open(os.path.join(csrc, "reverb.hip")).read()
    assert "atomic" not in kernel and "lt_philox" in kernel and "mfma_f32_32x32x2f32" in kernel and "mix_energy_sum" in kernel
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^FLAGS_reverb := -ffp-contract=off$", mk, re.M) and " reverb.hip " in mk


def _cfg(built, prob=0.5, normalize=1, align=1, max_taps=0, seed=1):
    return built.ReverbCfg(prob, normalize, align, max_taps, seed)


def test_size_helpers(built):
    lib = built.load()
    cfg = _cfg(built)
    pad = lambda v: (v + 255) // 256 * 256
    for n in (1, 6, 1000):
        assert lib.uvad_reverb_state_bytes(C.byref(cfg), n) == 256 + pad(8 * (n + 1)) + 2 * pad(4 * n)      # tables and delays, no taps
    for B in (1, 5, 256):
        assert lib.uvad_reverb_ws_bytes(B) == 256 + pad(16 * B)
    assert lib.uvad_reverb_state_bytes(None, 6) == 0 and lib.uvad_reverb_state_bytes(C.byref(cfg), 0) == 0
    for bad in (_cfg(built, prob=2.0), _cfg(built, prob=math.nan), _cfg(built, max_taps=-1)):
        assert lib.uvad_reverb_state_bytes(C.byref(bad), 6) == 0
    assert lib.uvad_reverb_ws_bytes(0) == 0 and lib.uvad_reverb_ws_bytes(-3) == 0


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    first = (C.c_int64 * 4)(0, 5, 6, 100)
    st, bank, a, b, ws = (C.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))     # never dereferenced
    nbytes = lib.uvad_reverb_state_bytes(C.byref(_cfg(built)), 3)
    try:
        def reset(cfg=None, state=st, n=nbytes, bk=bank, fs=first, n_rirs=3):
            return lib.uvad_reverb_reset(ctx, state, n, C.byref(cfg if cfg is not None else _cfg(built)), bk, fs, n_rirs, None)
        assert lib.uvad_reverb_reset(None, st, nbytes, C.byref(_cfg(built)), bank, first, 3, None) == E_ARG
        assert lib.uvad_reverb_reset(ctx, st, nbytes, None, bank, first, 3, None) == E_ARG and "cfg" in err()
        for p in (-0.5, 1.5, math.nan, math.inf):
            assert reset(_cfg(built, prob=p)) == E_ARG and "prob" in err(), p
        assert reset(_cfg(built, max_taps=-1)) == E_ARG and "max_taps" in err()
        assert reset(n_rirs=0) == E_ARG and "n_rirs" in err()
        assert reset(state=None) == E_ARG and reset(bk=None) == E_ARG and reset(fs=None) == E_ARG
        assert reset(state=C.c_void_p(0x10008)) == E_ARG and "aligned" in err()
        assert reset(bk=C.c_void_p(0x20002)) == E_ARG and "aligned" in err()
        assert reset(fs=(C.c_int64 * 4)(0, 5, 5, 100)) == E_ARG and "empty" in err()
        assert reset(fs=(C.c_int64 * 4)(0, 5, 3, 100)) == E_ARG and reset(fs=(C.c_int64 * 4)(1, 5, 6, 100)) == E_ARG
        assert reset(fs=(C.c_int64 * 4)(0, 5, 6, 7 + (1 << 20))) == E_ARG and "max_taps" in err()      # K_r above the limit, and not cut
        assert reset(n=nbytes - 1) == E_ARG and "state too small" in err()

        def step(apply, d_in=a, fmt=0, B=2, S=100, out=b, state=st, wsp=ws, plan=None):
            head, tail = (ctx, d_in, fmt, B, S, None, out, plan), (state, nbytes, wsp, 1 << 20, None)
            return lib.uvad_reverb_apply(*head, 0, 0, *tail) if apply else lib.uvad_reverb_step(*head, *tail)
        for apply in (False, True):
            for kw in ({"d_in": None}, {"out": None}, {"state": None}, {"wsp": None}, {"fmt": 2}, {"fmt": -1}, {"B": 0}, {"S": 0}, {"S": 1 << 31},
                       {"B": 1 << 20, "S": (1 << 31) - 1}, {"state": C.c_void_p(0x10004)}, {"wsp": C.c_void_p(0x50008)}, {"out": C.c_void_p(0x40002)},
                       {"fmt": 1, "d_in": C.c_void_p(0x30001)}, {"d_in": b}, {"fmt": 1, "d_in": b}, {"plan": C.c_void_p(0x60002)}):
                assert step(apply, **kw) == E_ARG, (apply, kw)
            assert step(apply, d_in=b) == E_ARG and "d_out == d_in" in err()
            assert step(apply) == E_STATE and "uvad_reverb_reset" in err()        # in range, but the state was never reset
    finally:
        lib.uvad_destroy(ctx)
