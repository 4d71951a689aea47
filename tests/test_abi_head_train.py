"""Checks of the head fine-tuning entry points (uvad_head_train_*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; the configuration struct; the refusals made before the library touches a device (CPU); and, on a GPU, the size helpers and every
refusal that needs a context with a model: nothing is enqueued by a refused call."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_head_train_configure", "uvad_head_train_param_count", "uvad_head_train_state_bytes", "uvad_head_train_ws_bytes",
         "uvad_head_train_reset", "uvad_head_train_grad", "uvad_head_train_apply", "uvad_head_train_read", "uvad_head_train_commit"]
E_ARG, E_STATE, E_UNSUPPORTED = -1, -3, -5
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _cfg(built, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, segment=0):
    return built.HeadTrainCfg(lr, beta1, beta2, eps, segment)


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
    assert built.SIGNATURES["uvad_head_train_state_bytes"][0] is C.c_size_t and built.SIGNATURES["uvad_head_train_ws_bytes"][0] is C.c_size_t
    assert built.SIGNATURES["uvad_head_train_param_count"][0] is C.c_int64 and len(built.SIGNATURES["uvad_head_train_grad"][1]) == 19
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", raw) and built.ABI_VERSION == 5      # appended: the number stays
    for name, value in (("MASTERS", 0), ("GRAD", 1), ("M", 2), ("V", 3), ("SCALARS", 4), ("SCALAR_WORDS", 8)):
        assert int(re.search(rf"#define UVAD_HEAD_TRAIN_{name} (\d+)", raw).group(1)) == value == getattr(built, "HEAD_TRAIN_" + name)
    for cite in ("training_step", "configure_optimizers", "torch.optim.Adam", "binary_cross_entropy", "uvad_get_taps", "uvad_finalize"):
        assert cite in raw[raw.index("Head fine-tuning on the device"):raw.index("uvad_head_train_commit(uvad_ctx")], cite   # what it replaces
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bhead_train\.hip\b", mk, re.M) and re.search(r"^FLAGS_head_train := .*-ffp-contract=off", mk, re.M)
    kernel = open(os.path.join(csrc, "head_train.hip")).read()
    for k in ("ht_gemm_kernel", "ht_cls_kernel", "ht_fold_kernel", "__builtin_amdgcn_mfma_f32_32x32x2f32", "fp contract(off)"):
        assert k in kernel
    # Adam and the read-out work on the state's blocks alone: one launcher for every family (optim.hip), none of its own and no launch here
    assert not re.search(r"\blaunch_\w+_train_(apply|read)\s*\(", kernel) and not re.search(r"hipLaunchKernelGGL\(\s*ht_adam_kernel", kernel)
    assert "asm" not in kernel and "atomic" not in re.sub(r"//.*", "", kernel)     # no atomics at all: the same calls give the same bits


def test_cfg_struct_matches_the_header(built):
    src = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} uvad_head_train_cfg;", src).group(1), flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int|float)\s+([\w\s,]+);", body):
        fields += [(t, n.strip()) for n in names.split(",")]
    assert fields == [("float", "lr"), ("float", "beta1"), ("float", "beta2"), ("float", "eps"), ("int", "segment")]
    assert [f[0] for f in built.HeadTrainCfg._fields_] == [n for _, n in fields] and C.sizeof(built.HeadTrainCfg) == 20


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    try:
        assert lib.uvad_head_train_state_bytes(ctx) == 0 and lib.uvad_head_train_ws_bytes(ctx, 2, 100) == 0 and lib.uvad_head_train_param_count(ctx) == 0
        assert lib.uvad_head_train_state_bytes(None) == 0 and lib.uvad_head_train_ws_bytes(None, 2, 100) == 0
        bad = [(dict(lr=0.0), "lr"), (dict(lr=-1e-3), "lr"), (dict(lr=math.nan), "lr"), (dict(lr=math.inf), "lr"),
               (dict(beta1=1.0), "beta1"), (dict(beta1=-0.1), "beta1"), (dict(beta1=math.nan), "beta1"),
               (dict(beta2=1.0), "beta2"), (dict(beta2=-0.1), "beta2"), (dict(beta2=math.inf), "beta2"),
               (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(eps=math.nan), "eps"),
               (dict(segment=-32), "segment"), (dict(segment=16), "segment"), (dict(segment=48), "segment"), (dict(segment=(1 << 14) + 32), "segment")]
        for kw, word in bad:
            assert lib.uvad_head_train_configure(ctx, C.byref(_cfg(built, **kw))) == E_ARG and word in err(), kw
        assert lib.uvad_head_train_configure(ctx, None) == E_ARG and lib.uvad_head_train_configure(None, C.byref(_cfg(built))) == E_ARG
        assert lib.uvad_head_train_configure(ctx, C.byref(_cfg(built))) == E_STATE and "model" in err()      # a context without a model
        assert lib.uvad_head_train_state_bytes(ctx) == 0
        # no configuration: every call on a state is refused, arguments first
        grad = lambda x=fake, B=2, T=100, gt=fake, ld_gt=100, dz=None, ld_dz=0, st=fake, w=fake: \
            lib.uvad_head_train_grad(ctx, x, B, T, None, gt, ld_gt, None, 0, dz, ld_dz, None, 0, None, st, 1 << 30, w, 1 << 30, None)
        for kw in ({"x": None}, {"st": None}, {"w": None}, {"B": 0}, {"T": 0}, {"B": 1 << 13, "T": (1 << 11) + 1}, {"gt": None}, {"ld_gt": 99},
                   {"dz": fake, "ld_dz": 99}):
            assert grad(**kw) == E_ARG, kw
        assert grad() == E_STATE and "uvad_head_train_configure" in err()
        assert lib.uvad_head_train_reset(ctx, None, 1 << 20, None) == E_ARG and lib.uvad_head_train_reset(ctx, fake, 1 << 20, None) == E_STATE
        assert lib.uvad_head_train_apply(ctx, None, 1 << 20, None) == E_ARG and lib.uvad_head_train_apply(ctx, fake, 1 << 20, None) == E_STATE
        assert lib.uvad_head_train_read(ctx, fake, 1 << 20, 0, None, None) == E_ARG and lib.uvad_head_train_read(ctx, fake, 1 << 20, 5, fake, None) == E_ARG
        assert lib.uvad_head_train_read(ctx, fake, 1 << 20, -1, fake, None) == E_ARG and lib.uvad_head_train_read(ctx, fake, 1 << 20, 4, fake, None) == E_STATE
        assert lib.uvad_head_train_commit(ctx, None, 1 << 20) == E_ARG and lib.uvad_head_train_commit(ctx, fake, 1 << 20) == E_STATE
    finally:
        lib.uvad_destroy(ctx)


def _ctx(built, model):
    lib = built.load()
    ctx = C.c_void_p()
    mc = built.ModelCfg(*model)
    code = lib.uvad_create(0, None, C.byref(mc), C.byref(ctx))
    return lib, ctx, code


@gpu
def test_unsupported_head_shapes_and_the_size_helpers(built):
    # (in_dim, hidden, layers, bidirectional, lin_hidden, lin_layers, slope)
    for model, word in (((64, 128, 1, 1, 128, 5, 0.01), "feed-forward layers"), ((64, 128, 1, 1, 48, 1, 0.01), "lin_hidden"),
                        ((64, 128, 1, 1, 288, 1, 0.01), "lin_hidden"), ((64, 128, 1, 1, 16, 2, 0.01), "lin_hidden"),
                        ((64, 128, 1, 1, 128, 2, 0.0), "leaky_slope"), ((64, 128, 1, 1, 128, 2, -0.5), "leaky_slope")):
        lib, ctx, code = _ctx(built, model)
        try:
            assert code == 0, lib.uvad_last_error(ctx)
            assert lib.uvad_head_train_configure(ctx, C.byref(_cfg(built))) == E_UNSUPPORTED and word in lib.uvad_last_error(ctx).decode(), model
            assert lib.uvad_head_train_state_bytes(ctx) == 0
        finally:
            lib.uvad_destroy(ctx)
    for model, P in (((64, 128, 4, 1, 128, 2, 0.01), 256 * 128 + 128 + 128 * 128 + 128 + 128 + 1), ((4, 32, 1, 1, 32, 0, -1.0), 64 + 1),
                     ((4, 128, 1, 0, 256, 4, 0.5), 128 * 256 + 256 + 3 * (256 * 256 + 256) + 256 + 1)):
        lib, ctx, code = _ctx(built, model)
        try:
            assert code == 0 and lib.uvad_head_train_configure(ctx, C.byref(_cfg(built, segment=64))) == 0, lib.uvad_last_error(ctx)
            Pp = (P + 63) // 64 * 64
            assert lib.uvad_head_train_param_count(ctx) == P and lib.uvad_head_train_state_bytes(ctx) == 256 + 16 * Pp
            H, L = (model[4], model[5]) if model[5] else (0, 0)
            al = lambda v: (v + 255) // 256 * 256

            def ws(B, T, seg):
                N = B * T
                return 256 + al(N) + al(4 * N) + al(4 * L * N * H) + 2 * al(4 * N * H if L else 0) + al(4 * ((N + seg - 1) // seg) * Pp) + al(8 * ((N + 255) // 256))
            for B, T in ((1, 1), (3, 129), (2, 301)):
                assert lib.uvad_head_train_ws_bytes(ctx, B, T) == ws(B, T, 64), (model, B, T)
            assert lib.uvad_head_train_configure(ctx, C.byref(_cfg(built))) == 0
            assert lib.uvad_head_train_ws_bytes(ctx, 256, 1000) == ws(256, 1000, 2048)                   # default segment 2048
            assert lib.uvad_head_train_ws_bytes(ctx, 0, 10) == 0 and lib.uvad_head_train_ws_bytes(ctx, 1, 0) == 0
            assert lib.uvad_head_train_ws_bytes(ctx, 1 << 13, (1 << 11) + 1) == 0
        finally:
            lib.uvad_destroy(ctx)


@gpu
def test_call_refusals_on_a_context_with_a_model(built):
    import torch
    lib, ctx, code = _ctx(built, (4, 32, 1, 1, 32, 1, 0.01))
    err = lambda: lib.uvad_last_error(ctx).decode()
    try:
        assert code == 0 and lib.uvad_head_train_configure(ctx, C.byref(_cfg(built, segment=32))) == 0
        state, ws = lib.uvad_head_train_state_bytes(ctx), lib.uvad_head_train_ws_bytes(ctx, 2, 100)
        buf = torch.zeros(state + ws + 4096, dtype=torch.uint8, device="cuda:0")
        st, w, x = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + (state + 255) // 256 * 256), C.c_void_p(buf.data_ptr())
        assert lib.uvad_head_train_reset(ctx, st, state - 1, None) == E_ARG and f"need {state} bytes" in err()
        assert lib.uvad_head_train_reset(ctx, st, state, None) == E_STATE and "uvad_finalize" in err()     # no finalized model
        grad = lambda x=x, B=2, T=100, gt=x, ld_gt=100, fw=None, ld_fw=0, dz=None, ld_dz=0, p=None, ld_p=0, st=st, nst=state, w=w, nw=ws: \
            lib.uvad_head_train_grad(ctx, x, B, T, None, gt, ld_gt, fw, ld_fw, dz, ld_dz, p, ld_p, None, st, nst, w, nw, None)
        for kw in ({"x": None}, {"st": None}, {"w": None}, {"B": 0}, {"T": 0}, {"gt": None}, {"ld_gt": 99}, {"fw": x, "ld_fw": 99},
                   {"dz": x, "ld_dz": 99}, {"p": x, "ld_p": 99}, {"nst": state - 1}, {"nw": ws - 1}):
            assert grad(**kw) == E_ARG, kw
        assert "need" in err()
        assert grad() == E_STATE and "uvad_head_train_reset" in err()              # arguments in order, but the state was never reset
        assert lib.uvad_head_train_apply(ctx, st, state, None) == E_STATE and lib.uvad_head_train_apply(ctx, st, state - 1, None) == E_ARG
        assert lib.uvad_head_train_read(ctx, st, state, 0, x, None) == E_STATE and lib.uvad_head_train_read(ctx, st, state - 1, 0, x, None) == E_ARG
        assert lib.uvad_head_train_commit(ctx, st, state) == E_STATE and lib.uvad_head_train_commit(ctx, st, state - 1) == E_ARG
        torch.cuda.synchronize()
        assert not buf.any()                                                       # nothing was enqueued
    finally:
        lib.uvad_destroy(ctx)
