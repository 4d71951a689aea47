"""CPU checks of the channel fusion's entry points (uvad_fuse_*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; the constants; the kernel file's conventions; the workspace size; every refusal, all of which are made before the library
touches a device; and the host layer's tables and validation.  Without a GPU uvad_fuse_configure validates, keeps the configuration and
then fails its upload with UVAD_E_HIP -- which is what lets the refusals of uvad_fuse and uvad_fuse_pick be checked here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"uvad_fuse_configure": 6, "uvad_fuse_ws_bytes": 3, "uvad_fuse": 19, "uvad_fuse_pick": 9}
E_ARG, E_HIP, E_STATE = -1, -2, -3


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_fuse_entries_in_header_binding_and_export_list(built):
    text = open(os.path.join(ROOT, "include", "uvad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]) == nargs, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_fuse_ws_bytes"][0] is C.c_size_t
    assert all(built.SIGNATURES[n][0] is C.c_int for n in ("uvad_fuse_configure", "uvad_fuse", "uvad_fuse_pick"))
    assert built.load().uvad_abi_version() == built.ABI_VERSION == 5                    # adding symbols does not move it
    assert int(re.search(r"#define UVAD_ABI_VERSION (\d+)", src).group(1)) == 5
    for name, value in (("MAX", built.FUSE_MAX), ("MEAN", built.FUSE_MEAN), ("VOTE", built.FUSE_VOTE)):
        assert int(re.search(rf"#define UVAD_FUSE_{name}\s+(\d+)", src).group(1)) == value
    assert (built.FUSE_MAX, built.FUSE_MEAN, built.FUSE_VOTE) == (0, 1, 2)
    assert int(re.search(r"#define UVAD_FUSE_MAX_MEMBERS\s+(\d+)", src).group(1)) == built.FUSE_MAX_MEMBERS == 255
    assert int(re.search(r"#define UVAD_FUSE_STATS_WORDS\s+(\d+)", src).group(1)) == built.FUSE_STATS_WORDS == 4
    assert C.sizeof(built.FuseCfg) == 12 and [f[0] for f in built.FuseCfg._fields_] == ["mode", "threshold", "decide"]
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bfuse\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "fuse.hip")).read()
    for k in ("fuse_kernel", "fuse_fold_kernel", "fuse_pick_kernel"):
        assert k in kernel
    assert "asm" not in kernel and "atomic" not in re.sub(r"//.*", "", kernel)      # no inline assembly; no atomics in the code (cuts.hip's convention)
    assert "__ballot" in kernel and "__popcll" in kernel
    for cite in ("other_vad_metrics.py:156-213", "src/datasets/", "mdm"):
        assert cite in text, cite


def _cfg(built, mode=0, thr=0.5, dec=0.5):
    return built.FuseCfg(mode, thr, dec)


def _configure(lib, ctx, q, first, members, weights=None, G=None):
    f = np.asarray(first, np.int32)
    m = np.asarray(members, np.int32)
    w = None if weights is None else np.asarray(weights, np.float32)
    return lib.uvad_fuse_configure(ctx, C.byref(q), f.ctypes.data, m.ctypes.data, w.ctypes.data if w is not None else None,
                                   len(first) - 1 if G is None else G)


def test_configure_refusals(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    try:
        q = _cfg(built)
        one = np.zeros(4, np.int32)
        assert lib.uvad_fuse_ws_bytes(ctx, 4, 100) == 0                                  # before configure
        fake = C.c_void_p(0x1000)
        assert lib.uvad_fuse(ctx, fake, 8, 4, 8, None, None, fake, 8, fake, None, None, 8, None, 8, None, fake, 1 << 20, None) == E_STATE
        assert "uvad_fuse_configure" in err()
        assert lib.uvad_fuse_pick(ctx, fake, 8, fake, fake, 4, fake, fake, None) == E_STATE and "uvad_fuse_configure" in err()
        assert lib.uvad_fuse_configure(ctx, None, one.ctypes.data, one.ctypes.data, None, 1) == E_ARG and "cfg" in err()
        assert lib.uvad_fuse_configure(ctx, C.byref(q), None, one.ctypes.data, None, 1) == E_ARG and "h_group_first" in err()
        assert lib.uvad_fuse_configure(ctx, C.byref(q), one.ctypes.data, None, None, 1) == E_ARG and "h_members" in err()
        assert lib.uvad_fuse_configure(None, C.byref(q), one.ctypes.data, one.ctypes.data, None, 1) == E_ARG
        for kw, word in ((dict(first=[0, 2], members=[0, 1], G=0), "G"), (dict(first=[0, 2], members=[0, 1], G=-1), "G"),
                         (dict(first=[1, 2], members=[0, 1]), "h_group_first[0]"), (dict(first=[0, 2, 1], members=[0, 1]), "non-decreasing"),
                         (dict(first=[0, 2, 2], members=[0, 1]), "1 .. 255 members"), (dict(first=[0, 0, 2], members=[0, 1]), "1 .. 255 members"),
                         (dict(first=[0, 256], members=list(range(256))), "1 .. 255 members"),
                         (dict(first=[0, 2], members=[0, -1]), "member index"),
                         (dict(first=[0, 2], members=[0, 1], weights=[1.0, float("nan")]), "weight"),
                         (dict(first=[0, 2], members=[0, 1], weights=[float("inf"), 1.0]), "weight"),
                         (dict(first=[0, 2], members=[0, 1], weights=[1.0, -0.5]), "weight"),
                         (dict(first=[0, 2, 4], members=[0, 1, 2, 3], weights=[1.0, 1.0, 0.0, 0.0]), "sum to 0")):
            assert _configure(lib, ctx, q, **kw) == E_ARG and word in err(), kw
        for bad, word in ((_cfg(built, 3), "mode"), (_cfg(built, -1), "mode"), (_cfg(built, 0, float("nan")), "threshold"),
                          (_cfg(built, 0, float("inf")), "threshold"), (_cfg(built, 1, 0.5, float("nan")), "decide"),
                          (_cfg(built, 2, 0.5, -float("inf")), "decide")):
            assert _configure(lib, ctx, bad, [0, 2], [0, 1]) == E_ARG and word in err(), word
        assert lib.uvad_fuse_ws_bytes(ctx, 4, 100) == 0                                  # a refused configure leaves nothing behind
        assert _configure(lib, ctx, q, [0, 255], list(range(255))) in (0, E_HIP)         # 255 members are allowed
    finally:
        lib.uvad_destroy(ctx)


def test_ws_bytes_and_call_refusals(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    try:
        # three groups over rows 0 .. 6, row 2 in two of them: N = 7 member slots, the largest member index 6
        code = _configure(lib, ctx, _cfg(built, 1), [0, 2, 5, 7], [0, 2, 2, 3, 6, 4, 5], [1, 1, 0, 2, 1, 1, 1])
        assert code in (0, E_HIP)                     # validated and kept; the upload needs a device
        ws = lambda B, T: lib.uvad_fuse_ws_bytes(ctx, B, T)
        # one 16-byte partial per member slot, 1024-frame tile and wave of the 256-thread workgroup
        assert [ws(7, 1), ws(7, 1024), ws(7, 1025), ws(100, 3001), ws(7, 1 << 30)] == [7 * 4 * 16, 7 * 4 * 16, 7 * 8 * 16, 7 * 12 * 16, 7 * (1 << 22) * 16]
        assert ws(6, 100) == 0 and ws(0, 100) == 0 and ws(7, 0) == 0 and ws(7, (1 << 30) + 1) == 0 and lib.uvad_fuse_ws_bytes(None, 7, 1) == 0
        need = ws(7, 100)

        def fuse(d_in=fake, ld_in=100, B=7, T=100, lens=fake, fl_in=None, fused=fake, ld_f=100, glens=fake, fl_out=None, labels=fake, ld_l=100,
                 best=fake, ld_b=100, stats=fake, w=fake, nw=need):
            return lib.uvad_fuse(ctx, d_in, ld_in, B, T, lens, fl_in, fused, ld_f, glens, fl_out, labels, ld_l, best, ld_b, stats, w, nw, None)
        for kw, word in (({"d_in": None}, "d_in"), ({"fused": None}, "d_fused"), ({"glens": None}, "d_glens"), ({"w": None}, "d_ws"),
                         ({"B": 6}, "largest configured member index (6)"), ({"B": 0}, "B"), ({"T": 0}, "T"), ({"T": (1 << 30) + 1, "nw": 1 << 62}, "T"),
                         ({"ld_in": 99}, "ld_in"), ({"ld_f": 99}, "ld_f"), ({"ld_l": 99}, "ld_l"), ({"ld_b": 99}, "ld_b"),
                         ({"nw": need - 1}, f"need {need} bytes"), ({"nw": 0}, f"need {need} bytes"),
                         ({"fl_in": fake}, "d_flags"), ({"fl_out": fake}, "d_flags")):
            assert fuse(**kw) == E_ARG and word in err(), kw
        if code == E_HIP:                             # no device: calls whose arguments are accepted stop at "not on the device" (with a
            # device they would be enqueued on these made-up pointers, so they are made only here); a leading dimension is checked only
            # where its array is given, and every optional output may be NULL
            assert fuse(labels=None, ld_l=0, best=None, ld_b=0, stats=None, lens=None) == E_HIP and "not on the device" in err()
            assert fuse(fl_in=fake, fl_out=fake) == E_HIP
        assert lib.uvad_fuse(None, fake, 100, 7, 100, None, None, fake, 100, fake, None, None, 0, None, 0, None, fake, need, None) == E_ARG

        def pick(best=fake, ld_b=100, table=fake, total=fake, max_cuts=8, out=fake, pk=fake):
            return lib.uvad_fuse_pick(ctx, best, ld_b, table, total, max_cuts, out, pk, None)
        for kw, word in (({"best": None}, "d_best"), ({"total": None}, "d_total"), ({"table": None}, "d_table"), ({"max_cuts": -1}, "max_cuts"),
                         ({"ld_b": 0}, "ld_b"), ({"out": None, "pk": None}, "both NULL")):
            assert pick(**kw) == E_ARG and word in err(), kw
        if code == E_HIP:
            assert pick(out=None) == E_HIP and pick(pk=None) == E_HIP and pick(table=None, max_cuts=0) == E_HIP     # either output may be NULL
        assert lib.uvad_fuse_pick(None, fake, 100, fake, fake, 8, fake, fake, None) == E_ARG
    finally:
        lib.uvad_destroy(ctx)


def test_host_tables_and_fuse_config(built):
    from uvad_amd.postprocess import fuse_config
    from uvad_amd.runtime import VadRuntime
    assert VadRuntime.FUSE_MODES == {"max": built.FUSE_MAX, "mean": built.FUSE_MEAN, "vote": built.FUSE_VOTE}
    assert VadRuntime.FUSE_STAT_NAMES == ("valid", "speech", "agree", "best")
    q = fuse_config(groups=[[0, 1], (2, 3, 4)])
    assert q == {"mode": "max", "threshold": 0.5, "decide": 0.5, "groups": [[0, 1], [2, 3, 4]], "weights": None}
    assert fuse_config("mean", 0.3)["decide"] == 0.3 and fuse_config("vote", 0.3)["decide"] == 0.5 and fuse_config("vote", 0.3, 0.2)["decide"] == 0.2
    assert fuse_config("mean", groups=[[0, 1]], weights=[[0, 2]])["weights"] == [[0.0, 2.0]]
    for bad in (dict(mode="median"), dict(threshold=float("nan")), dict(decide=float("inf")), dict(threshold="0.5"), dict(threshold=True),
                dict(groups=[]), dict(groups=[[]]), dict(groups=[list(range(256))]), dict(groups=[[0, -1]]), dict(weights=[[1.0]]),
                dict(groups=[[0, 1]], weights=[[1.0]]), dict(groups=[[0, 1]], weights=[[1.0, -1.0]]), dict(groups=[[0, 1]], weights=[[0.0, 0.0]]),
                dict(groups=[[0, 1]], weights=[[1.0, float("nan")]]), dict(groups=[[0, 1], [2]], weights=[[1.0, 1.0]])):
        with pytest.raises(ValueError):
            fuse_config(**bad)


def test_gate_with_fuse_is_refused_before_anything_is_allocated(built):
    from uvad_amd.runtime import VadRuntime
    st = {"B": 4, "out": None}
    with pytest.raises(ValueError, match="gate= together with fuse= is not built"):
        VadRuntime._slots_fuse(None, st, {"groups": [[0, 1], [2, 3]]}, {})
    assert VadRuntime._slots_fuse(None, st, None, {}) is None
    import inspect
    for opener in (VadRuntime.window_slots_open, VadRuntime.wav_window_slots_open):
        assert inspect.signature(opener).parameters["fuse"].default is None


def test_test_vad_still_refuses_all_channels_without_fuse(built):
    from uvad_amd.scripts import test_vad as run_test
    with pytest.raises(ValueError, match="one recording per file"):
        run_test(input={"kind": "wav", "paths": ["a.wav"], "labels": ["a.txt"], "channels": "all"}, feature_extractor="fbank")
