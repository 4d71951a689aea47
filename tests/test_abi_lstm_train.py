"""Checks of the LSTM training entry points (uvad_lstm_train_*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; the configuration struct; the refusals made before the library touches a device (CPU); and, on a GPU, the size helpers and every
refusal that needs a context with a model: nothing is enqueued by a refused call."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_lstm_train_configure", "uvad_lstm_train_param_count", "uvad_lstm_train_state_bytes", "uvad_lstm_train_ws_bytes",
         "uvad_lstm_train_reset", "uvad_lstm_train_forward", "uvad_lstm_train_backward", "uvad_lstm_train_apply", "uvad_lstm_train_read",
         "uvad_lstm_train_commit"]
E_ARG, E_STATE, E_UNSUPPORTED = -1, -3, -5
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _cfg(built, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, segment=0, first_layer=0):
    return built.LstmTrainCfg(lr, beta1, beta2, eps, segment, first_layer)


def test_entries_in_header_binding_and_export_list(built):
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_lstm_train_state_bytes"][0] is C.c_size_t and built.SIGNATURES["uvad_lstm_train_ws_bytes"][0] is C.c_size_t
    assert built.SIGNATURES["uvad_lstm_train_param_count"][0] is C.c_int64
    assert len(built.SIGNATURES["uvad_lstm_train_forward"][1]) == 11 and len(built.SIGNATURES["uvad_lstm_train_backward"][1]) == 12
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", raw) and built.ABI_VERSION == 5      # appended: the number stays
    block = raw[raw.index("LSTM training on the device"):raw.index("uvad_lstm_train_commit(uvad_ctx")]
    for cite in ("training_step", "configure_optimizers", "torch.optim.Adam", "pack_padded_sequence", "uvad_head_train_grad", "uvad_finalize",
                 "i, f, g, o", "dpre W_hh", "first_layer", "UVAD_E_UNSUPPORTED"):
        assert cite in block, cite
    assert raw.index("uvad_head_train_commit(uvad_ctx") < raw.index("LSTM training on the device")     # after the head's block
    head = raw[raw.index("Head fine-tuning on the device"):raw.index("uvad_head_train_commit(uvad_ctx")]
    assert "uvad_lstm_train_backward" in head                                   # the pointer from where d_grad_x is described
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\blstm_train\.hip\b", mk, re.M) and re.search(r"^FLAGS_lstm_train := .*-ffp-contract=off", mk, re.M)
    assert re.search(r"^%\.o:.*\bht_kernels\.h\b", mk, re.M)
    kernel = open(os.path.join(csrc, "lstm_train.hip")).read()
    for k in ("lt_fwd_kernel", "lt_bwd_kernel", "ht_gemm_kernel<0>", "ht_gemm_kernel<1>", "ht_gemm_kernel<2>", "ht_fold_kernel",
              "__builtin_amdgcn_mfma_f32_4x4x1f32", '#include "ht_kernels.h"'):
        assert k in kernel, k
    # Adam and the read-out work on the state's blocks alone: one launcher for every family (optim.hip), none of its own and no launch here
    assert not re.search(r"\blaunch_\w+_train_(apply|read)\s*\(", kernel) and not re.search(r"hipLaunchKernelGGL\(\s*ht_adam_kernel", kernel)
    assert "atomic" not in re.sub(r"//.*", "", kernel)                          # no atomics at all: the same calls give the same bits
    # one copy of the tile kernel: defined in the shared header, in neither file
    shared = open(os.path.join(csrc, "ht_kernels.h")).read()
    define = re.compile(r"void\s+ht_gemm_kernel\s*\(")
    assert len(define.findall(shared)) == 1 and "__builtin_amdgcn_mfma_f32_32x32x2f32(" in shared
    for fn in ("lstm_train.hip", "head_train.hip"):
        txt = open(os.path.join(csrc, fn)).read()
        assert not define.search(txt) and "__builtin_amdgcn_mfma_f32_32x32x2f32(" not in txt and '#include "ht_kernels.h"' in txt, fn


def test_cfg_struct_matches_the_header(built):
    src = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} uvad_lstm_train_cfg;", src).group(1), flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int|float)\s+([\w\s,]+);", body):
        fields += [(t, n.strip()) for n in names.split(",")]
    assert fields == [("float", "lr"), ("float", "beta1"), ("float", "beta2"), ("float", "eps"), ("int", "segment"), ("int", "first_layer")]
    assert [f[0] for f in built.LstmTrainCfg._fields_] == [n for _, n in fields] and C.sizeof(built.LstmTrainCfg) == 24


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    try:
        assert lib.uvad_lstm_train_state_bytes(ctx) == 0 and lib.uvad_lstm_train_ws_bytes(ctx, 2, 100) == 0 and lib.uvad_lstm_train_param_count(ctx) == 0
        assert lib.uvad_lstm_train_state_bytes(None) == 0 and lib.uvad_lstm_train_ws_bytes(None, 2, 100) == 0
        bad = [(dict(lr=0.0), "lr"), (dict(lr=-1e-3), "lr"), (dict(lr=math.nan), "lr"), (dict(lr=math.inf), "lr"),
               (dict(beta1=1.0), "beta1"), (dict(beta1=-0.1), "beta1"), (dict(beta1=math.nan), "beta1"),
               (dict(beta2=1.0), "beta2"), (dict(beta2=-0.1), "beta2"), (dict(beta2=math.inf), "beta2"),
               (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(eps=math.nan), "eps"),
               (dict(segment=-32), "segment"), (dict(segment=16), "segment"), (dict(segment=48), "segment"), (dict(segment=(1 << 14) + 32), "segment")]
        for kw, word in bad:
            assert lib.uvad_lstm_train_configure(ctx, C.byref(_cfg(built, **kw))) == E_ARG and word in err(), kw
        assert lib.uvad_lstm_train_configure(ctx, None) == E_ARG and lib.uvad_lstm_train_configure(None, C.byref(_cfg(built))) == E_ARG
        assert lib.uvad_lstm_train_configure(ctx, C.byref(_cfg(built))) == E_STATE and "model" in err()      # a context without a model
        assert lib.uvad_lstm_train_state_bytes(ctx) == 0
        # no configuration: every call on a state is refused, arguments first
        fwd = lambda x=fake, B=2, T=100, y=fake, st=fake, w=fake: lib.uvad_lstm_train_forward(ctx, x, B, T, None, y, st, 1 << 30, w, 1 << 30, None)
        bwd = lambda x=fake, dy=fake, B=2, T=100, st=fake, w=fake: lib.uvad_lstm_train_backward(ctx, x, dy, B, T, None, None, st, 1 << 30, w, 1 << 30, None)
        for kw in ({"x": None}, {"y": None}, {"st": None}, {"w": None}, {"B": 0}, {"T": 0}, {"B": 1 << 13, "T": (1 << 11) + 1}):
            assert fwd(**kw) == E_ARG, kw
        for kw in ({"x": None}, {"dy": None}, {"st": None}, {"w": None}, {"B": 0}, {"T": 0}, {"B": 1 << 13, "T": (1 << 11) + 1}):
            assert bwd(**kw) == E_ARG, kw
        assert fwd() == E_STATE and "uvad_lstm_train_configure" in err() and bwd() == E_STATE
        assert lib.uvad_lstm_train_reset(ctx, None, 1 << 20, None) == E_ARG and lib.uvad_lstm_train_reset(ctx, fake, 1 << 20, None) == E_STATE
        assert lib.uvad_lstm_train_apply(ctx, None, 1 << 20, None) == E_ARG and lib.uvad_lstm_train_apply(ctx, fake, 1 << 20, None) == E_STATE
        assert lib.uvad_lstm_train_read(ctx, fake, 1 << 20, 0, None, None) == E_ARG and lib.uvad_lstm_train_read(ctx, fake, 1 << 20, 5, fake, None) == E_ARG
        assert lib.uvad_lstm_train_read(ctx, fake, 1 << 20, -1, fake, None) == E_ARG and lib.uvad_lstm_train_read(ctx, fake, 1 << 20, 4, fake, None) == E_STATE
        assert lib.uvad_lstm_train_commit(ctx, None, 1 << 20) == E_ARG and lib.uvad_lstm_train_commit(ctx, fake, 1 << 20) == E_STATE
    finally:
        lib.uvad_destroy(ctx)


def _ctx(built, model):
    lib = built.load()
    ctx = C.c_void_p()
    mc = built.ModelCfg(*model)
    code = lib.uvad_create(0, None, C.byref(mc), C.byref(ctx))
    return lib, ctx, code


@pytest.mark.gpu
def test_unsupported_shapes_bad_first_layer_and_the_size_helpers(built):
    # (in_dim, hidden, layers, bidirectional, lin_hidden, lin_layers, slope)
    for model, first, code_want, word in (((64, 32, 1, 1, 32, 1, 0.01), 0, E_UNSUPPORTED, "hidden"), ((64, 256, 1, 1, 32, 1, 0.01), 0, E_UNSUPPORTED, "hidden"),
                                          ((64, 96, 2, 0, 32, 1, 0.01), 1, E_UNSUPPORTED, "hidden"),
                                          ((2052, 64, 1, 1, 32, 1, 0.01), 0, E_UNSUPPORTED, "2048"), ((64, 64, 9, 0, 32, 1, 0.01), 0, E_UNSUPPORTED, "8 trainable"),
                                          ((64, 64, 2, 1, 32, 1, 0.01), 2, E_ARG, "first_layer"), ((64, 64, 2, 1, 32, 1, 0.01), -1, E_ARG, "first_layer")):
        lib, ctx, code = _ctx(built, model)
        try:
            assert code == 0, lib.uvad_last_error(ctx)
            assert lib.uvad_lstm_train_configure(ctx, C.byref(_cfg(built, first_layer=first))) == code_want and word in lib.uvad_last_error(ctx).decode(), model
            assert lib.uvad_lstm_train_state_bytes(ctx) == 0
        finally:
            lib.uvad_destroy(ctx)
    al = lambda v: (v + 255) // 256 * 256
    for model, first in (((60, 64, 1, 1, 32, 1, 0.01), 0), ((60, 128, 3, 1, 32, 1, 0.01), 1), ((256, 128, 9, 0, 32, 0, 0.01), 1), ((4, 64, 2, 0, 32, 1, 0.01), 0)):
        lib, ctx, code = _ctx(built, model)
        try:
            assert code == 0 and lib.uvad_lstm_train_configure(ctx, C.byref(_cfg(built, segment=64, first_layer=first))) == 0, lib.uvad_last_error(ctx)
            Din0, H, L, D = model[0], model[1], model[2], 2 if model[3] else 1
            nl = L - first
            ins = [Din0 if first == 0 else H * D] + [H * D] * (nl - 1)
            P = sum(D * (4 * H * k + 4 * H * H + 8 * H) for k in ins)
            Pp = (P + 63) // 64 * 64
            assert lib.uvad_lstm_train_param_count(ctx) == P and lib.uvad_lstm_train_state_bytes(ctx) == 256 + 16 * Pp

            def ws(B, T, seg):
                N = B * T
                per = al(4 * D * N * 4 * H) + 2 * al(4 * D * N * H)
                return (512 + al(N) + al(4 * nl * D * 4 * H) + nl * per + (nl - 1) * al(4 * N * H * D) + 2 * al(4 * N * H * D if nl > 1 else 0) +
                        al(4 * ((N + seg - 1) // seg) * Pp))
            for B, T in ((1, 1), (5, 37), (9, 5)):
                assert lib.uvad_lstm_train_ws_bytes(ctx, B, T) == ws(B, T, 64), (model, B, T)
            assert lib.uvad_lstm_train_configure(ctx, C.byref(_cfg(built, first_layer=first))) == 0
            assert lib.uvad_lstm_train_ws_bytes(ctx, 16, 1000) == ws(16, 1000, 2048)                     # default segment 2048
            assert lib.uvad_lstm_train_ws_bytes(ctx, 0, 10) == 0 and lib.uvad_lstm_train_ws_bytes(ctx, 1, 0) == 0
            assert lib.uvad_lstm_train_ws_bytes(ctx, 1 << 13, (1 << 11) + 1) == 0
        finally:
            lib.uvad_destroy(ctx)


@pytest.mark.gpu
def test_call_refusals_on_a_context_with_a_model(built):
    import torch
    lib, ctx, code = _ctx(built, (4, 64, 1, 1, 32, 1, 0.01))
    err = lambda: lib.uvad_last_error(ctx).decode()
    try:
        assert code == 0 and lib.uvad_lstm_train_configure(ctx, C.byref(_cfg(built, segment=32))) == 0
        state, ws = lib.uvad_lstm_train_state_bytes(ctx), lib.uvad_lstm_train_ws_bytes(ctx, 2, 10)
        buf = torch.zeros(state + ws + 4096, dtype=torch.uint8, device="cuda:0")
        st, w, x = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + (state + 255) // 256 * 256), C.c_void_p(buf.data_ptr())
        assert lib.uvad_lstm_train_reset(ctx, st, state - 1, None) == E_ARG and f"need {state} bytes" in err()
        assert lib.uvad_lstm_train_reset(ctx, st, state, None) == E_STATE and "uvad_finalize" in err()     # no finalized model
        fwd = lambda x=x, B=2, T=10, y=x, st=st, nst=state, w=w, nw=ws: lib.uvad_lstm_train_forward(ctx, x, B, T, None, y, st, nst, w, nw, None)
        bwd = lambda x=x, dy=x, B=2, T=10, st=st, nst=state, w=w, nw=ws: lib.uvad_lstm_train_backward(ctx, x, dy, B, T, None, None, st, nst, w, nw, None)
        for kw in ({"x": None}, {"y": None}, {"st": None}, {"w": None}, {"B": 0}, {"T": 0}, {"nst": state - 1}, {"nw": ws - 1}):
            assert fwd(**kw) == E_ARG, kw
        for kw in ({"x": None}, {"dy": None}, {"st": None}, {"w": None}, {"B": 0}, {"T": 0}, {"nst": state - 1}, {"nw": ws - 1}):
            assert bwd(**kw) == E_ARG, kw
        assert "need" in err()
        assert fwd() == E_STATE and "uvad_lstm_train_reset" in err() and bwd() == E_STATE       # arguments in order, but the state was never reset
        assert lib.uvad_lstm_train_apply(ctx, st, state, None) == E_STATE and lib.uvad_lstm_train_apply(ctx, st, state - 1, None) == E_ARG
        assert lib.uvad_lstm_train_read(ctx, st, state, 0, x, None) == E_STATE and lib.uvad_lstm_train_read(ctx, st, state - 1, 0, x, None) == E_ARG
        assert lib.uvad_lstm_train_commit(ctx, st, state) == E_STATE and lib.uvad_lstm_train_commit(ctx, st, state - 1) == E_ARG
        torch.cuda.synchronize()
        assert not buf.any()                                                       # nothing was enqueued
    finally:
        lib.uvad_destroy(ctx)
