"""Checks of the sampler entry points (uvad_sampler_*, include/uvad.h) that need no GPU: declared, bound and exported; the struct layout;
the header's statement of the definitions; the size helpers; the refusals made before the library touches a device (fake device pointers
that are never dereferenced; the host tables are real).  The refusals that need a reset state are in test_gpu_sampler.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_sampler_state_bytes", "uvad_sampler_ws_bytes", "uvad_sampler_reset", "uvad_sampler_step", "uvad_sampler_apply", "uvad_sampler_read",
         "uvad_sampler_write"]
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
    step, apply = built.SIGNATURES["uvad_sampler_step"][1], built.SIGNATURES["uvad_sampler_apply"][1]
    assert apply[:9] == step[:9] and apply[12:] == step[9:] and apply[10] is C.c_int64 and apply[11] is C.c_uint64
    assert src.index("uvad_reverb_apply(") < src.index("uvad_sampler_state_bytes(")              # appended behind the augmentation blocks


def test_struct_layout_and_constants(built):
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} uvad_sampler_cfg;", raw).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in built.SamplerCfg._fields_] == ["window", "min_keep", "geometry", "half", "step", "shuffle", "drop_last", "pad",
                                                                   "batch", "seed"]
    assert C.sizeof(built.SamplerCfg) == 56 and built.SamplerCfg.geometry.offset == 16 and built.SamplerCfg.batch.offset == 40
    assert built.SamplerCfg.seed.offset == 48
    for name, val in (("UVAD_SAMPLER_FBANK", built.SAMPLER_FBANK), ("UVAD_SAMPLER_SINCNET", built.SAMPLER_SINCNET),
                      ("UVAD_SAMPLER_PLAN_WORDS", built.SAMPLER_PLAN_WORDS), ("UVAD_SAMPLER_MAX_SETS", built.SAMPLER_MAX_SETS)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", raw).group(1)) == val, name


def test_header_states_the_definitions():
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    block = raw[raw.index("Training batches drawn on the device"):raw.index("} uvad_sampler_cfg;")]
    for cite in ("n > min_keep", "k = max(8, bits(N - 1))", "cycle walking", "(R | t << 16, 0x53500000 | d, e_lo, e_hi)", "(seed_lo, seed_hi)",
                 "(row0 + b, 0x53440000, draw_lo, draw_hi)", "(uint64)w0 < cum[d]", "cum[D - 1] = 2^32", "L = floor(N / batch) batch",
                 "bit for bit", "q / 32768", "st = rs / hop, et = re / hop", "max(floordiv(rs - half, step), 0)", "re < len_b", "byte 56",
                 "{dataset, epoch (low word), position p, window, recording, start,", "No atomics", "UNPINNED",
                 "UVAD_E_STATE: a state that was never reset"):
        assert cite in block, cite
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    kernel = re.sub(r"//.*", "", open(os.path.join(csrc, "sampler.hip")).read())
    assert "atomic" not in kernel and "lt_philox" in kernel and "hipMalloc" not in kernel and "Synchronize" not in kernel
    assert " sampler.hip " in open(os.path.join(csrc, "Makefile")).read()


def _cfg(built, window=1000, min_keep=100, geometry=1, half=496, step=270, shuffle=1, drop_last=0, pad=0, batch=0, seed=1):
    return built.SamplerCfg(window, min_keep, geometry, half, step, shuffle, drop_last, pad, batch, seed)


def test_size_helpers(built):
    lib = built.load()
    pad = lambda v: (v + 255) // 256 * 256
    cfg = _cfg(built)
    for R, n_sup in ((1, 0), (7, 300), (1000, 12345)):
        want = 256 + 2048 + pad(4 * R) + pad(4 * (R + 1)) + pad(8 * (R + 1)) + pad(4 * (R + 1)) + pad(16 * n_sup)      # tables, no audio, no windows
        assert lib.uvad_sampler_state_bytes(C.byref(cfg), R, n_sup, 3) == want
    for B in (1, 5, 256):
        assert lib.uvad_sampler_ws_bytes(B) == 256 + pad(32 * B)
    assert lib.uvad_sampler_ws_bytes(0) == 0 and lib.uvad_sampler_state_bytes(None, 3, 0, 1) == 0
    sb = lambda R=3, n_sup=0, D=1, **kw: lib.uvad_sampler_state_bytes(C.byref(_cfg(built, **kw)), R, n_sup, D)
    assert sb() > 0 and sb(R=0) == 0 and sb(n_sup=-1) == 0 and sb(D=0) == 0 and sb(D=65) == 0 and sb(D=64) > 0
    assert sb(window=0) == 0 and sb(window=1 << 31) == 0 and sb(window=(1 << 31) - 1) > 0 and sb(min_keep=-1) == 0 and sb(min_keep=1000) == 0
    assert sb(geometry=2) == 0 and sb(step=0) == 0 and sb(half=-1) == 0 and sb(geometry=0, step=0, half=-1) > 0
    assert sb(drop_last=1, D=2) == 0 and sb(drop_last=1, batch=0) == 0 and sb(drop_last=1, batch=4) > 0


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    st, pcm, a, b, ws, lab, fr = (C.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000))     # never dereferenced
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    f64 = lambda *v: (C.c_double * len(v))(*v)
    first, sup, supf, sets, wts = i64(0, 2500, 2600, 6000), i64(0, 10, 5, 7), i32(0, 1, 1, 2), i32(0, 0, 1), f64(1.0, 2.0)
    nbytes = lib.uvad_sampler_state_bytes(C.byref(_cfg(built)), 3, 2, 2)
    try:
        def reset(cfg=None, state=st, n=nbytes, pc=pcm, fmt=0, fs=first, R=3, sp=sup, sf=supf, n_sup=2, rs=sets, w=wts, D=2, c=ctx):
            return lib.uvad_sampler_reset(c, state, n, C.byref(cfg) if cfg is not None else C.byref(_cfg(built)), pc, fmt, fs, R, sp, sf, n_sup, rs, w,
                                          D, None)
        assert reset(c=None) == E_ARG
        assert lib.uvad_sampler_reset(ctx, st, nbytes, None, pcm, 0, first, 3, sup, supf, 2, sets, wts, 2, None) == E_ARG and "cfg" in err()
        for kw in ({"state": None}, {"pc": None}, {"fs": None}, {"sf": None}, {"rs": None}, {"w": None}, {"sp": None}):
            assert reset(**kw) == E_ARG, kw
        for cfg, word in ((_cfg(built, window=0), "window"), (_cfg(built, window=1 << 31), "window"), (_cfg(built, min_keep=-1), "min_keep"),
                          (_cfg(built, min_keep=1000), "min_keep"), (_cfg(built, geometry=2), "geometry"), (_cfg(built, geometry=-1), "geometry"),
                          (_cfg(built, step=0), "step"), (_cfg(built, half=-1), "half"), (_cfg(built, drop_last=1, batch=4), "drop_last")):
            assert reset(cfg) == E_ARG and word in err(), word
        assert reset(_cfg(built, drop_last=1, batch=0), rs=i32(0, 0, 0), w=f64(1.0), D=1) == E_ARG and "batch" in err()
        assert reset(_cfg(built, drop_last=1, batch=9), rs=i32(0, 0, 0), w=f64(1.0), D=1) == E_ARG and "fewer windows" in err()   # N = 3 + 0 + 4
        assert reset(D=0) == E_ARG and "D" in err() and reset(D=65) == E_ARG
        assert reset(fmt=2) == E_ARG and "fmt" in err() and reset(fmt=-1) == E_ARG
        assert reset(R=0) == E_ARG and "R" in err() and reset(n_sup=-1) == E_ARG and "n_sup" in err()
        assert reset(state=C.c_void_p(0x10008)) == E_ARG and "aligned" in err()
        assert reset(pc=C.c_void_p(0x20002)) == E_ARG and "aligned" in err() and reset(pc=C.c_void_p(0x20001), fmt=1) == E_ARG
        assert reset(fs=i64(1, 2500, 2600, 6000)) == E_ARG and "h_rec_first[0]" in err()
        assert reset(fs=i64(0, 2500, 2500, 6000)) == E_ARG and "empty" in err()
        assert reset(fs=i64(0, 2500, 2400, 6000)) == E_ARG and "h_rec_first" in err()
        assert reset(fs=i64(0, 2500, 2600, 2600 + (1 << 31))) == E_ARG and "2^31 - 1" in err()
        assert reset(sf=i32(1, 1, 1, 2)) == E_ARG and "h_sup_first" in err() and reset(sf=i32(0, 1, 1, 3)) == E_ARG and "h_sup_first" in err()
        assert reset(sf=i32(0, 2, 1, 2)) == E_ARG and "h_sup_first" in err()
        assert reset(rs=i32(0, 2, 1)) == E_ARG and "dataset index" in err() and reset(rs=i32(0, -1, 1)) == E_ARG and "dataset index" in err()
        assert reset(rs=i32(0, 0, 0)) == E_ARG and "without windows" in err()                      # dataset 1 owns no recording
        assert reset(rs=i32(0, 1, 0)) == E_ARG and "without windows" in err()                      # ... or only one of 100 samples: not > min_keep
        for bad in (0.0, -1.0, math.nan, math.inf):
            assert reset(w=f64(1.0, bad)) == E_ARG and "weight" in err(), bad
        assert reset(n=nbytes - 1) == E_ARG and "state too small" in err()
        # in range: the geometry's configuration is what is missing (this context has neither a feature nor a SincNet configuration)
        assert reset() == E_STATE and "uvad_sincnet_configure" in err()
        assert reset(_cfg(built, geometry=0)) == E_STATE and "feature configuration" in err()

        def step(apply, B=2, out=a, ld_out=1000, ns=b, lb=lab, ld_gt=100, frames=fr, plan=None, cur=i64(0, 0), state=st, wsp=ws):
            head, tail = (ctx, B, out, ld_out, ns, lb, ld_gt, frames, plan), (state, nbytes, wsp, 1 << 20, None)
            return lib.uvad_sampler_apply(*head, cur, 0, 0, *tail) if apply else lib.uvad_sampler_step(*head, *tail)
        for apply in (False, True):
            for kw in ({"out": None}, {"ns": None}, {"lb": None}, {"frames": None}, {"state": None}, {"wsp": None}, {"B": 0}, {"B": -3},
                       {"state": C.c_void_p(0x10004)}, {"wsp": C.c_void_p(0x50008)}, {"out": C.c_void_p(0x30002)}, {"ns": C.c_void_p(0x40004)},
                       {"frames": C.c_void_p(0x70002)}, {"plan": C.c_void_p(0x80002)}):
                assert step(apply, **kw) == E_ARG, (apply, kw)
            assert step(apply) == E_STATE and "uvad_sampler_reset" in err()        # in range, but the state was never reset
        assert step(True, cur=None) == E_ARG
        rec = C.c_void_p(0x90000)
        assert lib.uvad_sampler_read(ctx, st, nbytes, None, None) == E_ARG and lib.uvad_sampler_write(ctx, st, nbytes, None, None) == E_ARG
        assert lib.uvad_sampler_read(ctx, None, nbytes, rec, None) == E_ARG and lib.uvad_sampler_write(ctx, None, nbytes, rec, None) == E_ARG
        assert lib.uvad_sampler_read(ctx, st, nbytes, rec, None) == E_STATE and "uvad_sampler_reset" in err()
        assert lib.uvad_sampler_write(ctx, st, nbytes, rec, None) == E_STATE and "uvad_sampler_reset" in err()
        assert lib.uvad_sampler_read(None, st, nbytes, rec, None) == E_ARG
    finally:
        lib.uvad_destroy(ctx)
