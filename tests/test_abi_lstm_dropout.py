"""Checks of the dropout entry points (uvad_lstm_train_set_dropout, uvad_dropout_apply, include/uvad.h): declared, bound and exported; the
header's definition of the mask; the refusals made before the library touches a device (CPU, fake pointers that are never dereferenced);
and, on a GPU, that the setting needs a configuration and changes neither size helper."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_lstm_train_set_dropout", "uvad_dropout_apply"]
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
    assert built.SIGNATURES["uvad_lstm_train_set_dropout"][1] == [C.c_void_p, C.c_float, C.c_uint64]
    assert built.SIGNATURES["uvad_dropout_apply"][1][2] is C.c_int64 and built.SIGNATURES["uvad_dropout_apply"][1][5] is C.c_uint64
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", raw) and built.ABI_VERSION == 5      # appended: the number stays
    block = raw[raw.index("LSTM training on the device"):raw.index("uvad_lstm_train_commit(uvad_ctx")]
    for cite in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "6627e8d5 e169c58d bc57ac4c 9b00dbd8",
                 "(n, (k << 16) | (j >> 2), draw_lo, draw_hi)", "(seed_lo, seed_hi)", "j & 3", "floor((double)p 2^32)", "1.0f / (1.0f - p)",
                 "word >= thr", "byte 56", "byte 16", "byte 24", "byte 28", "byte 32", "uvad_dropout_apply", "uvad_lstm_train_set_dropout"):
        assert cite in block, cite
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "lstm_train.hip")).read()
    assert "lt_dropout_kernel" in kernel and "atomic" not in re.sub(r"//.*", "", kernel)


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    try:
        assert lib.uvad_lstm_train_set_dropout(None, 0.5, 1) == E_ARG
        for p in (math.nan, math.inf, -math.inf, -0.1, 1.0, 1.5):
            assert lib.uvad_lstm_train_set_dropout(ctx, p, 1) == E_ARG and "[0, 1)" in err(), p
        for p in (0.0, 0.5, 0.999):                   # in range, but a context without a model, and no uvad_lstm_train_configure
            assert lib.uvad_lstm_train_set_dropout(ctx, p, 1) == E_STATE and "model" in err(), p
        assert lib.uvad_lstm_train_state_bytes(ctx) == 0 and lib.uvad_lstm_train_ws_bytes(ctx, 2, 100) == 0
    finally:
        lib.uvad_destroy(ctx)
    a, b = C.c_void_p(0x1000), C.c_void_p(0x2000)     # never dereferenced
    call = lambda x=a, out=b, rows=5, cols=8, layer=0, p=0.5: lib.uvad_dropout_apply(x, out, rows, cols, layer, 0, p, 1, None)
    for kw in ({"x": None}, {"out": None}, {"x": C.c_void_p(0x1004)}, {"out": C.c_void_p(0x2008)}, {"rows": 0}, {"rows": -1}, {"rows": (1 << 24) + 1},
               {"cols": 0}, {"cols": 6}, {"cols": -4}, {"cols": 2052}, {"layer": -1}, {"layer": 65536}, {"p": -0.1}, {"p": 1.0}, {"p": math.nan},
               {"p": math.inf}):
        assert call(**kw) == E_ARG, kw


@pytest.mark.gpu
def test_set_dropout_needs_a_configuration_and_changes_no_size(built):
    lib = built.load()
    ctx = C.c_void_p()
    mc = built.ModelCfg(16, 64, 3, 1, 32, 1, 0.01)
    assert lib.uvad_create(0, None, C.byref(mc), C.byref(ctx)) == 0
    try:
        assert lib.uvad_lstm_train_set_dropout(ctx, 0.5, 1) == E_STATE and "uvad_lstm_train_configure" in lib.uvad_last_error(ctx).decode()
        cfg = built.LstmTrainCfg(1e-3, 0.9, 0.999, 1e-8, 32, 0)
        assert lib.uvad_lstm_train_configure(ctx, C.byref(cfg)) == 0
        sizes = lambda: (lib.uvad_lstm_train_state_bytes(ctx), lib.uvad_lstm_train_ws_bytes(ctx, 5, 19), lib.uvad_lstm_train_param_count(ctx))
        before = sizes()
        for p in (0.5, 0.0, 0.3):
            assert lib.uvad_lstm_train_set_dropout(ctx, p, 0xFFFFFFFFFFFFFFFF) == 0 and sizes() == before
        assert lib.uvad_lstm_train_set_dropout(ctx, 1.0, 1) == E_ARG
        assert lib.uvad_lstm_train_configure(ctx, C.byref(cfg)) == 0 and sizes() == before
    finally:
        lib.uvad_destroy(ctx)
