"""Checks of the joint optimizer step's entry points (uvad_optim_*, and the _write calls of the three training families, include/uvad.h):
declared in the header, bound in the ctypes table and exported; the configuration struct; every refusal made before the library touches a
device (CPU); and, on a GPU, the byte helpers and the refusals that need a context with a model: nothing is enqueued by a refused call."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_optim_state_bytes", "uvad_optim_ws_bytes", "uvad_optim_reset", "uvad_optim_set_lr_table", "uvad_optim_step", "uvad_optim_read",
         "uvad_optim_write", "uvad_head_train_write", "uvad_lstm_train_write", "uvad_sincnet_train_write"]
E_ARG, E_STATE = -1, -3
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _cfg(built, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, weight_decay=0.0, decoupled=0, skip_nonfinite=0, lr_scale=(1.0, 1.0, 1.0)):
    return built.OptimCfg(beta1, beta2, eps, max_norm, weight_decay, decoupled, skip_nonfinite, (C.c_float * 3)(*lr_scale))


def _table(*v):
    return (C.c_float * len(v))(*v)


def test_entries_in_header_binding_and_export_list(built):
    raw = open(os.path.join(ROOT, "include", "uvad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_optim_state_bytes"][0] is C.c_size_t and built.SIGNATURES["uvad_optim_ws_bytes"][0] is C.c_size_t
    assert len(built.SIGNATURES["uvad_optim_step"][1]) == 12
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", raw) and built.ABI_VERSION == 5      # appended: the number stays
    assert int(re.search(r"#define UVAD_OPTIM_RECORD_WORDS (\d+)", raw).group(1)) == 8 == built.OPTIM_RECORD_WORDS
    assert int(re.search(r"#define UVAD_LSTM_TRAIN_SCALAR_WORDS (\d+)", raw).group(1)) == 10 == built.LSTM_TRAIN_SCALAR_WORDS
    assert int(re.search(r"#define UVAD_HEAD_TRAIN_SCALAR_WORDS (\d+)", raw).group(1)) == 8                  # the head's record did not move
    section = raw[raw.index("The joint optimizer step on the device"):raw.index("uvad_sincnet_train_write(uvad_ctx")]
    for cite in ("clip_grad_norm_", "AdamW", "vad_engine.py:275", "uvad_optim_set_lr_table", "DDP is not here", "chunk order"):
        assert cite in section, cite
    for part in ("Head fine-tuning on the device", "LSTM training on the device", "SincNet training on the device"):
        assert "uvad_optim_step, below" in raw[raw.index(part):raw.index(part) + 6000], part              # the "not here" sentences point here
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\boptim\.hip\b", mk, re.M) and re.search(r"^FLAGS_optim := .*-ffp-contract=off", mk, re.M)
    kernel = open(os.path.join(csrc, "optim.hip")).read()
    for k in ("opt_sumsq_kernel", "opt_fold_kernel", "opt_adam_kernel", "opt_commit_kernel", "ht_adam_kernel", "ht_adam_commit_kernel", "ht_read_kernel",
              "ht_write_kernel", "ht_state_ok"):
        assert k in kernel
    # one launcher each for the three families' _apply, _read and _write: defined once under csrc/, and that is here
    every = {fn: open(os.path.join(csrc, fn)).read() for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".h"))}
    for name in ("launch_train_apply", "launch_train_read", "launch_train_write"):
        define = re.compile(rf"hipError_t\s+{name}\s*\([^;{{]*\)\s*\{{")
        assert sum(len(define.findall(txt)) for txt in every.values()) == 1 and define.search(kernel), name
    assert "asm" not in kernel and "atomic" not in re.sub(r"//.*", "", kernel)      # no atomics at all: the same calls give the same bits


def test_cfg_struct_matches_the_header(built):
    src = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} uvad_optim_cfg;", src).group(1), flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int|float)\s+([\w\s,\[\]]+);", body):
        fields += [(t, n.strip()) for n in names.split(",")]
    assert fields == [("float", "beta1"), ("float", "beta2"), ("float", "eps"), ("float", "max_norm"), ("float", "weight_decay"),
                      ("int", "decoupled"), ("int", "skip_nonfinite"), ("float", "lr_scale[3]")]
    assert [f[0] for f in built.OptimCfg._fields_] == [n.split("[")[0] for _, n in fields] and C.sizeof(built.OptimCfg) == 40


def test_byte_helper_of_the_state_needs_no_context(built):
    lib = built.load()
    for n, want in ((1, 256 + 256), (64, 256 + 256), (65, 256 + 512), (1000, 256 + 16 * 256), (1 << 24, 256 + 4 * (1 << 24))):
        assert lib.uvad_optim_state_bytes(n) == want, n
    assert lib.uvad_optim_state_bytes(0) == 0 and lib.uvad_optim_state_bytes(-3) == 0 and lib.uvad_optim_state_bytes((1 << 24) + 1) == 0
    assert lib.uvad_optim_ws_bytes(None) == 0


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    big = 1 << 20
    try:
        assert lib.uvad_optim_ws_bytes(ctx) == 0                                  # no family configured
        ok_t = _table(1e-3, 5e-4)
        reset = lambda st=fake, n=big, cfg=None, t=ok_t, n_lr=2, **kw: \
            lib.uvad_optim_reset(ctx, st, n, C.byref(cfg if cfg is not None else _cfg(built, **kw)), t, n_lr, None)
        assert lib.uvad_optim_reset(ctx, fake, big, None, ok_t, 2, None) == E_ARG and "cfg" in err()
        assert lib.uvad_optim_reset(None, fake, big, C.byref(_cfg(built)), ok_t, 2, None) == E_ARG
        assert reset(st=None) == E_ARG
        assert lib.uvad_optim_reset(ctx, fake, big, C.byref(_cfg(built)), None, 2, None) == E_ARG and "h_lr_table" in err()
        for n_lr in (0, -1, (1 << 24) + 1):
            assert reset(n_lr=n_lr) == E_ARG and "n_lr" in err(), n_lr
        for v in (0.0, -1e-3, math.nan, math.inf):
            assert reset(t=_table(1e-3, v)) == E_ARG and "table entry" in err(), v
        bad = [(dict(beta1=1.0), "beta1"), (dict(beta1=-0.1), "beta1"), (dict(beta1=math.nan), "beta1"),
               (dict(beta2=1.0), "beta2"), (dict(beta2=-0.1), "beta2"), (dict(beta2=math.inf), "beta2"),
               (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(eps=math.nan), "eps"),
               (dict(max_norm=-1.0), "max_norm"), (dict(max_norm=math.nan), "max_norm"), (dict(max_norm=math.inf), "max_norm"),
               (dict(weight_decay=-1e-2), "weight_decay"), (dict(weight_decay=math.nan), "weight_decay"),
               (dict(lr_scale=(1.0, -0.5, 1.0)), "lr_scale"), (dict(lr_scale=(1.0, 1.0, math.nan)), "lr_scale"), (dict(lr_scale=(math.inf, 1.0, 1.0)), "lr_scale")]
        for kw, word in bad:
            assert reset(**kw) == E_ARG and word in err(), kw
        assert reset(n=lib.uvad_optim_state_bytes(2) - 1) == E_ARG and "need 512 bytes" in err()
        assert reset(st=C.c_void_p(0x1004)) == E_ARG and "aligned" in err()
        # a state that was never reset: every call on it is refused, arguments first
        assert lib.uvad_optim_set_lr_table(ctx, None, big, ok_t, 2, None) == E_ARG and lib.uvad_optim_set_lr_table(ctx, fake, big, None, 2, None) == E_ARG
        assert lib.uvad_optim_set_lr_table(ctx, fake, big, ok_t, 0, None) == E_ARG and lib.uvad_optim_set_lr_table(ctx, fake, big, _table(0.0), 1, None) == E_ARG
        assert lib.uvad_optim_set_lr_table(ctx, fake, big, ok_t, 2, None) == E_STATE and "uvad_optim_reset" in err()
        assert lib.uvad_optim_read(ctx, fake, big, None, None) == E_ARG and lib.uvad_optim_read(ctx, None, big, fake, None) == E_ARG
        assert lib.uvad_optim_read(ctx, fake, big, fake, None) == E_STATE
        assert lib.uvad_optim_write(ctx, fake, big, None, None) == E_ARG and lib.uvad_optim_write(ctx, fake, big, fake, None) == E_STATE
        step = lambda h=fake, l=None, s=None, o=fake, w=fake: lib.uvad_optim_step(ctx, h, big, l, big, s, big, o, big, w, big, None)
        assert step(o=None) == E_ARG and step(w=None) == E_ARG
        assert step(h=None) == E_ARG and "at least one" in err()                   # all three states NULL
        assert lib.uvad_optim_step(None, fake, big, None, 0, None, 0, fake, big, fake, big, None) == E_ARG
        for kw, word in ((dict(), "uvad_head_train_configure"), (dict(h=None, l=fake), "uvad_lstm_train_configure"),
                         (dict(h=None, s=fake), "uvad_sincnet_train_configure")):
            assert step(**kw) == E_STATE and word in err(), kw                    # a family whose state is given is not configured
        for name in ("head", "lstm", "sincnet"):
            fn = getattr(lib, f"uvad_{name}_train_write")
            assert fn(ctx, fake, big, 0, None, None) == E_ARG and fn(None, fake, big, 0, fake, None) == E_ARG
            for which in (-1, 1, 5):                                              # _GRAD is not written
                assert fn(ctx, fake, big, which, fake, None) == E_ARG, (name, which)
            assert fn(ctx, None, big, 0, fake, None) == E_ARG
            assert fn(ctx, fake, big, 4, fake, None) == E_STATE and f"uvad_{name}_train_configure" in err()
    finally:
        lib.uvad_destroy(ctx)


@gpu
def test_size_helpers_and_call_refusals_on_a_context_with_a_model(built):
    import torch
    lib = built.load()
    ctx = C.c_void_p()
    mc = built.ModelCfg(80, 64, 2, 1, 32, 1, 0.01)      # (in_dim, hidden, layers, bidirectional, lin_hidden, lin_layers, slope)
    assert lib.uvad_create(0, None, C.byref(mc), C.byref(ctx)) == 0
    err = lambda: lib.uvad_last_error(ctx).decode()
    try:
        assert lib.uvad_optim_ws_bytes(ctx) == 0
        assert lib.uvad_head_train_configure(ctx, C.byref(built.HeadTrainCfg(1e-3, 0.9, 0.999, 1e-8, 32))) == 0
        Ph = int(lib.uvad_head_train_param_count(ctx))
        al = lambda v: (v + 255) // 256 * 256
        chunks = lambda P: (P + 4095) // 4096
        assert Ph == 128 * 32 + 32 + 32 + 1 and lib.uvad_optim_ws_bytes(ctx) == al(8 * chunks(Ph)) == 256
        assert lib.uvad_lstm_train_configure(ctx, C.byref(built.LstmTrainCfg(1e-3, 0.9, 0.999, 1e-8, 32, 0))) == 0
        Pl = int(lib.uvad_lstm_train_param_count(ctx))
        assert Pl == 174080 and lib.uvad_optim_ws_bytes(ctx) == al(8 * (chunks(Ph) + chunks(Pl))) == 512
        nh, nl, no = lib.uvad_head_train_state_bytes(ctx), lib.uvad_lstm_train_state_bytes(ctx), lib.uvad_optim_state_bytes(4)
        buf = torch.zeros(nh + nl + no + 4096, dtype=torch.uint8, device="cuda:0")
        base = buf.data_ptr()
        hs, ls, os_, ws = (C.c_void_p(base), C.c_void_p(base + al(nh)), C.c_void_p(base + al(nh) + al(nl)),
                           C.c_void_p(base + al(nh) + al(nl) + al(no)))
        nws = lib.uvad_optim_ws_bytes(ctx)
        step = lambda h=hs, bh=nh, l=ls, bl=nl, o=os_, bo=no, w=ws, bw=nws: lib.uvad_optim_step(ctx, h, bh, l, bl, None, 0, o, bo, w, bw, None)
        assert step(bh=nh - 1) == E_ARG and "need" in err() and step(bl=nl - 1) == E_ARG
        assert step() == E_STATE and "uvad_optim_reset" in err()                   # the optim state was never reset
        torch.cuda.synchronize()
        assert not buf.any()                                                       # nothing was enqueued so far
        table = _table(1e-3, 2e-3, 3e-3, 4e-3)
        assert lib.uvad_optim_reset(ctx, os_, no, C.byref(_cfg(built)), table, 4, None) == 0, err()
        assert step(bo=no - 1) == E_ARG and step(bw=nws - 1) == E_ARG and "workspace too small" in err()
        assert step(w=C.c_void_p(ws.value + 4)) == E_ARG
        assert step() == E_STATE and "uvad_head_train_reset" in err()              # the family states were never reset
        assert step(h=None, bh=0) == E_STATE and "uvad_lstm_train_reset" in err()
        assert lib.uvad_optim_set_lr_table(ctx, os_, no, _table(*([1e-3] * 5)), 5, None) == E_ARG and "above" in err()
        assert lib.uvad_optim_set_lr_table(ctx, os_, no - 1, table, 4, None) == E_ARG
        assert lib.uvad_optim_read(ctx, os_, no - 1, ws, None) == E_ARG and lib.uvad_optim_write(ctx, os_, no - 1, ws, None) == E_ARG
        assert lib.uvad_head_train_write(ctx, hs, nh, 0, ws, None) == E_STATE and lib.uvad_head_train_write(ctx, hs, nh - 1, 0, ws, None) == E_ARG
        assert lib.uvad_lstm_train_write(ctx, ls, nl, 4, ws, None) == E_STATE and lib.uvad_lstm_train_write(ctx, ls, nl - 1, 4, ws, None) == E_ARG
        torch.cuda.synchronize()
        state = buf[al(nh) + al(nl):al(nh) + al(nl) + no].clone()
        assert not buf[:al(nh) + al(nl)].any() and not buf[al(nh) + al(nl) + no:].any()   # only the reset wrote, and only the optim state
        hd = state[:256].cpu().numpy()
        assert hd[:4].tobytes() == b"POVU" and hd[4:12].view("<i4").tolist() == [4, 4] and hd[64:80].view("<u8").tolist() == [0, 0]
        assert state[256:272].cpu().numpy().view("<f4").tolist() == [float(v) for v in table] and not state[272:].any()
        # a shorter table: accepted, and the record of a state that has not stepped reads as zeros
        assert lib.uvad_optim_set_lr_table(ctx, os_, no, _table(7e-3), 1, None) == 0
        assert lib.uvad_optim_read(ctx, os_, no, ws, None) == 0
        torch.cuda.synchronize()
        assert buf[al(nh) + al(nl) + 8:al(nh) + al(nl) + 12].cpu().numpy().view("<i4")[0] == 1      # n in use
        assert not buf[al(nh) + al(nl) + al(no):].any()
    finally:
        lib.uvad_destroy(ctx)
