"""Checks of the SincNet training entry points (uvad_sincnet_train_*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; the configuration struct; the refusals made before the library touches a device (CPU); and, on a GPU, the parameter counts
42 602 / 42 360 / 18 180, the size helpers and every refusal that needs a context with a SincNet stage: nothing is enqueued by a refused call."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_sincnet_train_configure", "uvad_sincnet_train_param_count", "uvad_sincnet_train_state_bytes", "uvad_sincnet_train_ws_bytes",
         "uvad_sincnet_train_reset", "uvad_sincnet_train_forward", "uvad_sincnet_train_backward", "uvad_sincnet_train_apply",
         "uvad_sincnet_train_read", "uvad_sincnet_train_commit"]
E_ARG, E_STATE, E_UNSUPPORTED = -1, -3, -5
REF_SINC = (10, 80, 251, 60, 5, 60, 5, 0.01, 1e-5)      # stride, n_filters, kernel_size, c2, k2, c3, k3, leaky_slope, eps
REF_MODEL = (60, 64, 1, 1, 32, 1, 0.01)                 # in_dim, hidden, layers, bidirectional, lin_hidden, lin_layers, slope


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _cfg(built, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, segment=0, first_stage=0):
    return built.SincNetTrainCfg(lr, beta1, beta2, eps, segment, first_stage)


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
    assert built.SIGNATURES["uvad_sincnet_train_state_bytes"][0] is C.c_size_t and built.SIGNATURES["uvad_sincnet_train_ws_bytes"][0] is C.c_size_t
    assert built.SIGNATURES["uvad_sincnet_train_param_count"][0] is C.c_int64
    assert built.SIGNATURES["uvad_sincnet_train_ws_bytes"][1][2] is C.c_int64 and built.SIGNATURES["uvad_sincnet_train_forward"][1][3] is C.c_int64
    assert len(built.SIGNATURES["uvad_sincnet_train_forward"][1]) == 10 and len(built.SIGNATURES["uvad_sincnet_train_backward"][1]) == 10
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", raw) and built.ABI_VERSION == 5      # appended: the number stays
    assert re.search(r"#define\s+UVAD_SINCNET_TRAIN_FILTERS\s+5\b", raw) and built.SINCNET_TRAIN_FILTERS == 5
    block = raw[raw.index("SincNet training on the device"):raw.index("uvad_sincnet_train_commit(uvad_ctx")]
    for cite in ("training_step", "configure_optimizers", "torch.optim.Adam", "ParamSincFB.filters()", "LOWEST index", "sign(+-0) = 0",
                 "torch.clamp", "uvad_lstm_train_backward", "uvad_finalize", "first_stage", "wav_norm1d.weight", "42602 / 42360 / 18180",
                 "dF = g G + b0 D", "PLAIN form", "UVAD_E_UNSUPPORTED", "magic word"):
        assert cite in block, cite
    assert raw.index("uvad_lstm_train_commit(uvad_ctx") < raw.index("SincNet training on the device")     # after the LSTM's block
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\blstm_train\.hip sincnet_train\.hip\b", mk, re.M) and re.search(r"^FLAGS_sincnet_train := .*-ffp-contract=off", mk, re.M)
    kernel = open(os.path.join(csrc, "sincnet_train.hip")).read()
    for k in ("st_bank_kernel", "st_conv_kernel", "st_wgrad_kernel", "st_dgrad_kernel", "st_norm_bwd_kernel", "st_bank_bwd_kernel", "ht_fold_kernel",
              "__builtin_amdgcn_mfma_f32_32x32x2f32(", '#include "ht_kernels.h"'):
        assert k in kernel, k
    # Adam and the read-out work on the state's blocks alone: one launcher for every family (optim.hip), none of its own and no launch here
    assert not re.search(r"\blaunch_\w+_train_(apply|read)\s*\(", kernel) and not re.search(r"hipLaunchKernelGGL\(\s*(ht_adam_kernel|ht_read_kernel)", kernel)
    assert "atomic" not in re.sub(r"//.*", "", kernel)                          # no atomics at all: the same calls give the same bits


def test_cfg_struct_matches_the_header(built):
    src = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} uvad_sincnet_train_cfg;", src).group(1), flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int|float)\s+([\w\s,]+);", body):
        fields += [(t, n.strip()) for n in names.split(",")]
    assert fields == [("float", "lr"), ("float", "beta1"), ("float", "beta2"), ("float", "eps"), ("int", "segment"), ("int", "first_stage")]
    assert [f[0] for f in built.SincNetTrainCfg._fields_] == [n for _, n in fields] and C.sizeof(built.SincNetTrainCfg) == 24


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    try:
        assert lib.uvad_sincnet_train_state_bytes(ctx) == 0 and lib.uvad_sincnet_train_ws_bytes(ctx, 2, 8000) == 0
        assert lib.uvad_sincnet_train_param_count(ctx) == 0
        assert lib.uvad_sincnet_train_state_bytes(None) == 0 and lib.uvad_sincnet_train_ws_bytes(None, 2, 8000) == 0
        bad = [(dict(lr=0.0), "lr"), (dict(lr=-1e-3), "lr"), (dict(lr=math.nan), "lr"), (dict(lr=math.inf), "lr"),
               (dict(beta1=1.0), "beta1"), (dict(beta1=-0.1), "beta1"), (dict(beta1=math.nan), "beta1"),
               (dict(beta2=1.0), "beta2"), (dict(beta2=-0.1), "beta2"), (dict(beta2=math.inf), "beta2"),
               (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(eps=math.nan), "eps"),
               (dict(segment=-32), "segment"), (dict(segment=16), "segment"), (dict(segment=48), "segment"), (dict(segment=(1 << 14) + 32), "segment"),
               (dict(first_stage=-1), "first_stage"), (dict(first_stage=3), "first_stage")]
        for kw, word in bad:
            assert lib.uvad_sincnet_train_configure(ctx, C.byref(_cfg(built, **kw))) == E_ARG and word in err(), kw
        assert lib.uvad_sincnet_train_configure(ctx, None) == E_ARG and lib.uvad_sincnet_train_configure(None, C.byref(_cfg(built))) == E_ARG
        assert lib.uvad_sincnet_train_configure(ctx, C.byref(_cfg(built))) == E_STATE and "model" in err()      # a context without a model
        assert lib.uvad_sincnet_train_state_bytes(ctx) == 0
        # no configuration: every call on a state is refused, arguments first
        fwd = lambda x=fake, B=2, S=8000, y=fake, st=fake, w=fake: lib.uvad_sincnet_train_forward(ctx, x, B, S, y, st, 1 << 30, w, 1 << 30, None)
        bwd = lambda x=fake, dy=fake, B=2, S=8000, st=fake, w=fake: lib.uvad_sincnet_train_backward(ctx, x, dy, B, S, st, 1 << 30, w, 1 << 30, None)
        for kw in ({"x": None}, {"y": None}, {"st": None}, {"w": None}, {"B": 0}, {"S": 0}, {"st": C.c_void_p(0x1008)}, {"w": C.c_void_p(0x1004)}):
            assert fwd(**kw) == E_ARG, kw
        for kw in ({"x": None}, {"dy": None}, {"st": None}, {"w": None}, {"B": 0}, {"S": 0}, {"st": C.c_void_p(0x1008)}, {"w": C.c_void_p(0x1004)}):
            assert bwd(**kw) == E_ARG, kw
        assert fwd() == E_STATE and "uvad_sincnet_train_configure" in err() and bwd() == E_STATE
        assert lib.uvad_sincnet_train_reset(ctx, None, 1 << 20, None) == E_ARG and lib.uvad_sincnet_train_reset(ctx, fake, 1 << 20, None) == E_STATE
        assert lib.uvad_sincnet_train_apply(ctx, None, 1 << 20, None) == E_ARG and lib.uvad_sincnet_train_apply(ctx, fake, 1 << 20, None) == E_STATE
        assert lib.uvad_sincnet_train_read(ctx, fake, 1 << 20, 0, None, None) == E_ARG and lib.uvad_sincnet_train_read(ctx, fake, 1 << 20, 6, fake, None) == E_ARG
        assert lib.uvad_sincnet_train_read(ctx, fake, 1 << 20, -1, fake, None) == E_ARG and lib.uvad_sincnet_train_read(ctx, fake, 1 << 20, 5, fake, None) == E_STATE
        assert lib.uvad_sincnet_train_commit(ctx, None, 1 << 20) == E_ARG and lib.uvad_sincnet_train_commit(ctx, fake, 1 << 20) == E_STATE
    finally:
        lib.uvad_destroy(ctx)


def _ctx(built, model=REF_MODEL, sinc=REF_SINC):
    lib = built.load()
    ctx = C.c_void_p()
    mc = built.ModelCfg(*model)
    code = lib.uvad_create(0, None, C.byref(mc), C.byref(ctx))
    if code == 0 and sinc is not None:
        sc = built.SincNetCfg(*sinc)
        code = lib.uvad_sincnet_configure(ctx, C.byref(sc))
    return lib, ctx, code


def _geo(S, sinc=REF_SINC):
    stride, nf, ks, c2, k2, c3, k3 = sinc[:7]
    L0 = (S - ks) // stride + 1 if S >= ks else 0
    Lp0 = L0 // 3
    L1 = Lp0 - k2 + 1 if Lp0 >= k2 else 0
    Lp1 = L1 // 3
    L2 = Lp1 - k3 + 1 if Lp1 >= k3 else 0
    return (L0, L1, L2), (Lp0, Lp1, L2 // 3)


@pytest.mark.gpu
def test_parameter_counts_unsupported_shapes_and_the_size_helpers(built):
    lib, ctx, code = _ctx(built, sinc=None)
    try:
        assert code == 0 and lib.uvad_sincnet_train_configure(ctx, C.byref(_cfg(built))) == E_STATE and "SincNet" in lib.uvad_last_error(ctx).decode()
    finally:
        lib.uvad_destroy(ctx)
    for sinc, first, want, word in (((10, 80, 251, 60, 5, 60, 5, 1.5, 1e-5), 0, E_UNSUPPORTED, "leaky_slope"),
                                    ((10, 80, 250, 60, 5, 60, 5, 0.01, 1e-5), 0, E_UNSUPPORTED, "odd"),
                                    ((10, 80, 250, 60, 5, 60, 5, 0.01, 1e-5), 1, 0, "")):
        lib, ctx, code = _ctx(built, sinc=sinc)
        try:
            assert code == 0, lib.uvad_last_error(ctx)
            assert lib.uvad_sincnet_train_configure(ctx, C.byref(_cfg(built, first_stage=first))) == want and word in lib.uvad_last_error(ctx).decode()
            assert (lib.uvad_sincnet_train_state_bytes(ctx) == 0) == (want != 0)
        finally:
            lib.uvad_destroy(ctx)
    al = lambda v: (v + 255) // 256 * 256
    p64 = lambda v: (v + 63) // 64 * 64
    lib, ctx, code = _ctx(built)
    try:
        assert code == 0
        for first, P in ((0, 42602), (1, 42360), (2, 18180)):
            assert lib.uvad_sincnet_train_configure(ctx, C.byref(_cfg(built, segment=64, first_stage=first))) == 0, lib.uvad_last_error(ctx)
            Pp = p64(P)
            assert lib.uvad_sincnet_train_param_count(ctx) == P
            assert lib.uvad_sincnet_train_state_bytes(ctx) == 256 + 4 * (4 * Pp + p64(80 * 251) + p64(42602) + 2 * p64(125))

            def ws(B, S, seg):
                _, Lp = _geo(S)
                C_ = (80, 60, 60)
                nseg = (B * 3 * Lp[first] + seg - 1) // seg
                GS = p64(80 * 251 + 80)
                per = sum(al(4 * B * C_[s] * Lp[s]) + al(B * C_[s] * Lp[s]) + al(8 * B * C_[s]) + (al(4 * B * C_[s] * Lp[s]) if s >= first else 0)
                          for s in range(3))
                return 512 + al(16 * B) + per + al(8 * B * 80) + al(4 * nseg * Pp) + (al(4 * nseg * GS) + al(4 * GS) if first == 0 else 0)
            for B, S in ((1, 991), (2, 2071), (3, 8000), (2, 4003)):
                assert lib.uvad_sincnet_train_ws_bytes(ctx, B, S) == ws(B, S, 64), (first, B, S)
            assert lib.uvad_sincnet_train_configure(ctx, C.byref(_cfg(built, first_stage=first))) == 0
            assert lib.uvad_sincnet_train_ws_bytes(ctx, 16, 80000) == ws(16, 80000, 2048)                 # default segment 2048
            assert lib.uvad_sincnet_train_ws_bytes(ctx, 0, 8000) == 0 and lib.uvad_sincnet_train_ws_bytes(ctx, 1, 0) == 0
            assert lib.uvad_sincnet_train_ws_bytes(ctx, 1, 990) == 0                                      # no frame
            assert lib.uvad_sincnet_train_ws_bytes(ctx, 65536, 991) == 0
            assert lib.uvad_sincnet_train_ws_bytes(ctx, 65535, 1 << 20) == 0                              # B L_0 above 2^31 - 1
        assert lib.uvad_sincnet_train_configure(ctx, C.byref(_cfg(built, segment=32))) == 0
        assert lib.uvad_sincnet_train_ws_bytes(ctx, 300, 80000) == 0                                      # more than 65535 segments
    finally:
        lib.uvad_destroy(ctx)


@pytest.mark.gpu
def test_call_refusals_on_a_context_with_a_sincnet_stage(built):
    import torch
    lib, ctx, code = _ctx(built)
    err = lambda: lib.uvad_last_error(ctx).decode()
    try:
        assert code == 0 and lib.uvad_sincnet_train_configure(ctx, C.byref(_cfg(built, segment=32))) == 0
        state, ws = lib.uvad_sincnet_train_state_bytes(ctx), lib.uvad_sincnet_train_ws_bytes(ctx, 2, 2071)
        buf = torch.zeros(state + ws + 4096, dtype=torch.uint8, device="cuda:0")
        st, w, x = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + (state + 255) // 256 * 256), C.c_void_p(buf.data_ptr())
        assert lib.uvad_sincnet_train_reset(ctx, st, state - 1, None) == E_ARG and f"need {state} bytes" in err()
        assert lib.uvad_sincnet_train_reset(ctx, st, state, None) == E_STATE and "uvad_finalize" in err()     # no finalized model
        fwd = lambda x=x, B=2, S=2071, y=x, st=st, nst=state, w=w, nw=ws: lib.uvad_sincnet_train_forward(ctx, x, B, S, y, st, nst, w, nw, None)
        bwd = lambda x=x, dy=x, B=2, S=2071, st=st, nst=state, w=w, nw=ws: lib.uvad_sincnet_train_backward(ctx, x, dy, B, S, st, nst, w, nw, None)
        for kw in ({"x": None}, {"y": None}, {"st": None}, {"w": None}, {"B": 0}, {"S": 0}, {"S": 990}, {"B": 65536}, {"nst": state - 1}, {"nw": ws - 1}):
            assert fwd(**kw) == E_ARG, kw
        for kw in ({"x": None}, {"dy": None}, {"st": None}, {"w": None}, {"B": 0}, {"S": 0}, {"S": 990}, {"B": 65536}, {"nst": state - 1}, {"nw": ws - 1}):
            assert bwd(**kw) == E_ARG, kw
        assert "need" in err()
        assert fwd() == E_STATE and "uvad_sincnet_train_reset" in err() and bwd() == E_STATE    # arguments in order, but the state was never reset
        assert lib.uvad_sincnet_train_apply(ctx, st, state, None) == E_STATE and lib.uvad_sincnet_train_apply(ctx, st, state - 1, None) == E_ARG
        assert lib.uvad_sincnet_train_read(ctx, st, state, 0, x, None) == E_STATE and lib.uvad_sincnet_train_read(ctx, st, state - 1, 0, x, None) == E_ARG
        assert lib.uvad_sincnet_train_commit(ctx, st, state) == E_STATE and lib.uvad_sincnet_train_commit(ctx, st, state - 1) == E_ARG
        torch.cuda.synchronize()
        assert not buf.any()                                                       # nothing was enqueued
    finally:
        lib.uvad_destroy(ctx)
