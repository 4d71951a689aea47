"""Checks of the noise-mixing entry points (uvad_mix_*, include/uvad.h) that need no GPU: declared, bound and exported; the struct layout;
the header's statement of the order and the coordinates; the size helpers; the refusals made before the library touches a device (fake
pointers that are never dereferenced)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_mix_state_bytes", "uvad_mix_ws_bytes", "uvad_mix_reset", "uvad_mix_step", "uvad_mix_apply"]
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
    step, apply = built.SIGNATURES["uvad_mix_step"][1], built.SIGNATURES["uvad_mix_apply"][1]
    assert step[4] is C.c_int64 and apply[8] is C.c_int64 and apply[9] is C.c_uint64 and apply[:8] == step[:8] and apply[10:] == step[8:]
    assert src.index("uvad_sincnet_train_commit(") < src.index("uvad_mix_state_bytes(")          # appended behind the training blocks


def test_struct_layout_and_constants(built):
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} uvad_mix_cfg;", raw).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in built.MixCfg._fields_] == ["mix_prob", "snr_steps", "h_amp", "max_seg", "seed"]
    assert C.sizeof(built.MixCfg) == 32 and built.MixCfg.h_amp.offset == 8 and built.MixCfg.max_seg.offset == 16 and built.MixCfg.seed.offset == 24
    for name, val in (("UVAD_MIX_MAX_SEG", built.MIX_MAX_SEG), ("UVAD_MIX_PLAN_HEAD", built.MIX_PLAN_HEAD), ("UVAD_MIX_SEG_WORDS", built.MIX_SEG_WORDS),
                      ("UVAD_INGEST_F32", built.INGEST_F32), ("UVAD_INGEST_I16", built.INGEST_I16)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", raw).group(1)) == val, name


def test_header_states_the_order_and_the_coordinates():
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    block = raw[raw.index("Noise mixing of training batches"):raw.index("} uvad_mix_cfg;")]
    for cite in ("(i / 4) mod 1024", "in increasing i", "o = 32, 16, 8, 4, 2, 1", "o = 8, 4, 2, 1", "No floating-point atomics", "WHOLE clip",
                 "Philox4x32-10", "(row b, segment k, draw_lo, draw_hi)", "(seed_lo,", "(uint64)w0 < floor(mix_prob 2^32)", "q = (w1 Q) >> 32",
                 "clip = (w2 n_clips) >> 32", "word 3 is reserved", "min(clip length, len_b - offset)", "(float)(amp[q] sqrt(E_row / E_clip))",
                 "+0 when E_clip == 0 or E_row == 0", "fl32(x + fl32(gain noise))", "no fused multiply-add", "byte 56", "q / 32768",
                 "{clip, dst offset, count, gain", "does not depend on the bank's size", "UVAD_E_STATE: a state that was never reset"):
        assert cite in block, cite
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    kernel = re.sub(r"//.*", "", open(os.path.join(csrc, "mix.hip")).read())
    assert "atomic" not in kernel and "lt_philox" in kernel and "fma" not in kernel
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^FLAGS_mix := -ffp-contract=off$", mk, re.M) and " mix.hip " in mk
    assert "lt_philox" in open(os.path.join(csrc, "philox.h")).read() and '#include "philox.h"' in open(os.path.join(csrc, "lstm_train.hip")).read()


def _cfg(built, amp, mix_prob=0.5, max_seg=8, seed=1):
    return built.MixCfg(mix_prob, len(amp), amp.ctypes.data_as(C.POINTER(C.c_double)), max_seg, seed)


def test_size_helpers(built):
    lib = built.load()
    amp = np.full(1024, 0.1)
    cfg = _cfg(built, amp)
    pad = lambda v: (v + 255) // 256 * 256
    for n in (1, 6, 1000):
        assert lib.uvad_mix_state_bytes(C.byref(cfg), n) == 256 + pad(8 * (n + 1)) + pad(8 * n) + pad(8 * 1024)      # tables and energies, no audio
    for B, ms in ((1, 1), (5, 8), (256, 64)):
        assert lib.uvad_mix_ws_bytes(B, ms) == 256 + pad(8 * B) + pad(4 * B * (4 + 4 * ms))
    assert lib.uvad_mix_state_bytes(None, 6) == 0 and lib.uvad_mix_state_bytes(C.byref(cfg), 0) == 0
    assert lib.uvad_mix_state_bytes(C.byref(_cfg(built, amp, mix_prob=2.0)), 6) == 0
    assert lib.uvad_mix_ws_bytes(0, 8) == 0 and lib.uvad_mix_ws_bytes(5, 0) == 0 and lib.uvad_mix_ws_bytes(5, 65) == 0


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    amp = np.full(4, 0.1)
    first = (C.c_int64 * 4)(0, 5, 6, 100)
    st, bank, a, b, ws = (C.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))     # never dereferenced
    nbytes = lib.uvad_mix_state_bytes(C.byref(_cfg(built, amp)), 3)
    try:
        def reset(cfg=None, state=st, n=nbytes, bk=bank, fs=first, n_clips=3):
            return lib.uvad_mix_reset(ctx, state, n, C.byref(cfg if cfg is not None else _cfg(built, amp)), bk, fs, n_clips, None)
        assert lib.uvad_mix_reset(None, st, nbytes, C.byref(_cfg(built, amp)), bank, first, 3, None) == E_ARG
        assert lib.uvad_mix_reset(ctx, st, nbytes, None, bank, first, 3, None) == E_ARG and "cfg" in err()
        for p in (-0.5, 1.5, math.nan, math.inf):
            assert reset(_cfg(built, amp, mix_prob=p)) == E_ARG and "mix_prob" in err(), p
        assert reset(built.MixCfg(0.5, 0, amp.ctypes.data_as(C.POINTER(C.c_double)), 8, 1)) == E_ARG and "snr_steps" in err()
        for bad in (-0.1, math.nan, math.inf):
            t = amp.copy()
            t[2] = bad
            assert reset(_cfg(built, t)) == E_ARG and "amplitude" in err(), bad
        for ms in (0, -1, 65):
            assert reset(_cfg(built, amp, max_seg=ms)) == E_ARG and "max_seg" in err(), ms
        assert reset(n_clips=0) == E_ARG and "n_clips" in err()
        assert reset(state=None) == E_ARG and reset(bk=None) == E_ARG and reset(fs=None) == E_ARG
        assert reset(state=C.c_void_p(0x10008)) == E_ARG and "aligned" in err()
        assert reset(fs=(C.c_int64 * 4)(0, 5, 5, 100)) == E_ARG and "empty" in err()
        assert reset(fs=(C.c_int64 * 4)(0, 5, 3, 100)) == E_ARG and reset(fs=(C.c_int64 * 4)(1, 5, 6, 100)) == E_ARG
        assert reset(n=nbytes - 1) == E_ARG and "state too small" in err()

        def step(apply, d_in=a, fmt=0, B=2, S=100, out=b, state=st, wsp=ws, plan=None):
            head, tail = (ctx, d_in, fmt, B, S, None, out, plan), (state, nbytes, wsp, 1 << 20, None)
            return lib.uvad_mix_apply(*head, 0, 0, *tail) if apply else lib.uvad_mix_step(*head, *tail)
        for apply in (False, True):
            for kw in ({"d_in": None}, {"out": None}, {"state": None}, {"wsp": None}, {"fmt": 2}, {"fmt": -1}, {"B": 0}, {"S": 0}, {"S": 1 << 31},
                       {"state": C.c_void_p(0x10004)}, {"wsp": C.c_void_p(0x50008)}, {"out": C.c_void_p(0x40002)}, {"fmt": 1, "d_in": C.c_void_p(0x30001)},
                       {"fmt": 1, "d_in": b}, {"plan": C.c_void_p(0x60002)}):
                assert step(apply, **kw) == E_ARG, (apply, kw)
            assert step(apply) == E_STATE and "uvad_mix_reset" in err()        # in range, but the state was never reset
    finally:
        lib.uvad_destroy(ctx)
