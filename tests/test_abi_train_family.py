"""What the three training families (uvad_head_train_*, uvad_lstm_train_*, uvad_sincnet_train_*, include/uvad.h) must keep identical,
because one copy of the host code serves them: the range checks of the optimiser's configuration with their words and their order, and the
order in which _apply, _read, _write and _commit refuse a state -- NULL, family not configured, too small, never reset -- each naming the
family's own entry.  The first two need no device; "too small" and "never reset" need a configured family, so a context with a model: a GPU."""
import ctypes as C
import math

import pytest

E_ARG, E_STATE = -1, -3
SINC = (10, 80, 251, 60, 5, 60, 5, 0.01, 1e-5)         # stride, n_filters, kernel_size, c2, k2, c3, k3, leaky_slope, eps
MODEL = (60, 64, 1, 0, 32, 1, 0.01)                    # in_dim, hidden, layers, bidirectional, lin_hidden, lin_layers, slope
FAMILIES = ("head", "lstm", "sincnet")
UNIT = {"head": "frames", "lstm": "frames", "sincnet": "positions"}   # what a segment counts


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _cfg(built, family, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, segment=0, own=0):
    """The family's configuration; own: first_layer / first_stage (the head has no field of its own)."""
    if family == "head":
        return built.HeadTrainCfg(lr, beta1, beta2, eps, segment)
    return (built.LstmTrainCfg if family == "lstm" else built.SincNetTrainCfg)(lr, beta1, beta2, eps, segment, own)


def _calls(lib, ctx, family, out):
    """{entry: call(state, state_bytes)} of the four calls on a state the families share; out: a non-NULL d_out / d_in."""
    fn = lambda op: getattr(lib, f"uvad_{family}_train_{op}")
    return {"apply": lambda st, n: fn("apply")(ctx, st, n, None),
            "read": lambda st, n: fn("read")(ctx, st, n, 4, out, None),
            "write": lambda st, n: fn("write")(ctx, st, n, 4, out, None),
            "commit": lambda st, n: fn("commit")(ctx, st, n)}


LR, B1, B2, EPS = "lr must be finite and positive", "beta1 must lie in [0, 1)", "beta2 must lie in [0, 1)", "eps must be finite and positive"
SEG = "segment must be 0 or a multiple of 32 in [32, 16384] "
BAD = [(dict(lr=0.0), LR), (dict(lr=-1e-3), LR), (dict(lr=math.nan), LR), (dict(lr=math.inf), LR),
       (dict(beta1=1.0), B1), (dict(beta1=-0.1), B1), (dict(beta1=math.nan), B1), (dict(beta1=math.inf), B1),
       (dict(beta2=1.0), B2), (dict(beta2=-0.1), B2), (dict(beta2=math.nan), B2), (dict(beta2=math.inf), B2),
       (dict(eps=0.0), EPS), (dict(eps=-1e-8), EPS), (dict(eps=math.nan), EPS), (dict(eps=math.inf), EPS),
       (dict(segment=-32), SEG), (dict(segment=16), SEG), (dict(segment=48), SEG), (dict(segment=(1 << 14) + 32), SEG),
       # the order: lr, beta1, beta2, eps, segment, then the family's own field
       (dict(lr=0.0, beta1=1.0, beta2=1.0, eps=0.0, segment=16, own=-1), LR), (dict(beta1=1.0, beta2=1.0, eps=0.0, segment=16, own=-1), B1),
       (dict(beta2=1.0, eps=0.0, segment=16, own=-1), B2), (dict(eps=0.0, segment=16, own=-1), EPS), (dict(segment=16, own=-1), SEG)]


@pytest.mark.parametrize("family", FAMILIES)
def test_shared_refusals_made_before_a_device_is_touched(built, family):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no model: without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    big = 1 << 20
    configure = getattr(lib, f"uvad_{family}_train_configure")
    try:
        for kw, words in BAD:
            want = f"uvad_{family}_train_configure: " + words + (UNIT[family] if words is SEG else "")
            assert configure(ctx, C.byref(_cfg(built, family, **kw))) == E_ARG and err() == want, (kw, err())
        for name, call in _calls(lib, ctx, family, fake).items():
            assert call(None, big) == E_ARG and err() == f"uvad_{family}_train_{name}: bad argument", name      # arguments first
            assert call(fake, big) == E_STATE and f"uvad_{family}_train_{name}: call uvad_{family}_train_configure first" == err(), name
            assert call(fake, 0) == E_STATE and f"uvad_{family}_train_configure" in err(), name                  # ... before any size
        given = {f: (fake if f == family else None) for f in FAMILIES}
        assert lib.uvad_optim_step(ctx, given["head"], big, given["lstm"], big, given["sincnet"], big, fake, big, fake, big, None) == E_STATE
        assert err() == f"uvad_optim_step: call uvad_{family}_train_configure first"
    finally:
        lib.uvad_destroy(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_shared_refusals_of_a_configured_family(built, family):
    import torch
    lib = built.load()
    ctx = C.c_void_p()
    assert lib.uvad_create(0, None, C.byref(built.ModelCfg(*MODEL)), C.byref(ctx)) == 0
    err = lambda: lib.uvad_last_error(ctx).decode()
    try:
        assert lib.uvad_sincnet_configure(ctx, C.byref(built.SincNetCfg(*SINC))) == 0, err()
        assert getattr(lib, f"uvad_{family}_train_configure")(ctx, C.byref(_cfg(built, family, segment=32))) == 0, err()
        need = getattr(lib, f"uvad_{family}_train_state_bytes")(ctx)
        assert need > 256
        buf = torch.zeros(need + 256, dtype=torch.uint8, device="cuda:0")
        st, out = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + need)
        for name, call in _calls(lib, ctx, family, out).items():
            assert call(None, need) == E_ARG and err() == f"uvad_{family}_train_{name}: bad argument", name
            assert call(st, need - 1) == E_ARG and err() == f"uvad_{family}_train_{name}: state too small: need {need} bytes", name
            assert call(st, need) == E_STATE and err() == f"uvad_{family}_train_{name}: call uvad_{family}_train_reset on this state first", name
        torch.cuda.synchronize()
        assert not buf.any()                                                       # nothing was enqueued
    finally:
        lib.uvad_destroy(ctx)
