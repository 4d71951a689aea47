"""CPU checks of the hysteresis entry points (uvad_binarize*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; the record; the workspace size; and every refusal, all of which are made before the library touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_binarize_ws_bytes", "uvad_binarize"]
E_ARG = -1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _cfg(built, onset=0.6, offset=0.4, min_on=5, min_off=3, pad_on=1, pad_off=2):
    return built.BinarizeCfg(onset, offset, min_on, min_off, pad_on, pad_off)


def test_binarize_entries_in_header_binding_and_export_list(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_binarize_ws_bytes"][0] is C.c_size_t and len(built.SIGNATURES["uvad_binarize"][1]) == 15
    assert built.load().uvad_abi_version() == built.ABI_VERSION == 5                # new symbols are found by name; the number did not move
    assert int(re.search(r"#define UVAD_ABI_VERSION (\d+)", src).group(1)) == 5
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bbinarize\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "binarize.hip")).read()
    for k in ("binarize_classify_kernel", "binarize_rows_kernel", "launch_intervals_to_labels", "float4"):
        assert k in kernel
    assert "asm" not in kernel and "atomic" not in re.sub(r"//.*", "", kernel)      # no inline assembly; no atomics in the code


def test_record_matches_the_header(built):
    src = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} uvad_binarize_cfg;", src).group(1), flags=re.S)
    fields = re.findall(r"\b(float|int)\s+(\w+);", body)
    assert [f[1] for f in fields] == ["onset", "offset", "min_on", "min_off", "pad_on", "pad_off"] == [f[0] for f in built.BinarizeCfg._fields_]
    assert [f[0] for f in fields] == ["float"] * 2 + ["int"] * 4
    assert [f[1] for f in built.BinarizeCfg._fields_] == [C.c_float] * 2 + [C.c_int] * 4 and C.sizeof(built.BinarizeCfg) == 24


BIG = (1 << 20) + 1
BAD_CFGS = [({"onset": float("nan")}, "onset"), ({"onset": float("inf")}, "onset"), ({"offset": float("nan")}, "offset"),
            ({"offset": float("-inf")}, "offset"), ({"onset": 0.3, "offset": 0.5}, "offset"),
            ({"min_on": -1}, "min_on"), ({"min_on": BIG}, "min_on"), ({"min_off": -1}, "min_off"), ({"min_off": BIG}, "min_off"),
            ({"pad_on": -1}, "pad_on"), ({"pad_on": BIG}, "pad_on"), ({"pad_off": -1}, "pad_off"), ({"pad_off": BIG}, "pad_off")]


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    try:
        # (T + 63) / 64 word pairs of 16 bytes and (T + 1) / 2 intervals of 8 bytes per row
        assert [lib.uvad_binarize_ws_bytes(ctx, B, T) for B, T in ((1, 1), (2, 9), (3, 1000), (1, 360000), (256, 1000))] == \
            [16 + 8, 2 * (16 + 5 * 8), 3 * (16 * 16 + 500 * 8), 5625 * 16 + 180000 * 8, 256 * (16 * 16 + 500 * 8)]
        assert lib.uvad_binarize_ws_bytes(ctx, 0, 10) == 0 and lib.uvad_binarize_ws_bytes(ctx, 1, 0) == 0
        assert lib.uvad_binarize_ws_bytes(None, 1, 1) == 0 and lib.uvad_binarize_ws_bytes(ctx, 1, (1 << 30) + 1) == 0
        assert lib.uvad_binarize_ws_bytes(ctx, 1, 1 << 30) == (1 << 24) * 16 + (1 << 29) * 8
        ws = lib.uvad_binarize_ws_bytes(ctx, 4, 100)
        good = _cfg(built)

        def call(p=fake, ld_p=100, B=4, T=100, q=good, lab=fake, ld=100, iv=fake, max_iv=8, cn=fake, w=fake, nw=ws):
            return lib.uvad_binarize(ctx, p, ld_p, B, T, None, C.byref(q) if q is not None else None, lab, ld, iv, max_iv, cn, w, nw, None)
        for kw, word in BAD_CFGS:
            assert call(q=_cfg(built, **kw)) == E_ARG and word in err(), kw
        assert call(q=None) == E_ARG and "cfg" in err()
        for kw, word in (({"B": 0}, "B"), ({"T": 0}, "T"), ({"T": (1 << 30) + 1, "ld_p": (1 << 30) + 1, "ld": (1 << 30) + 1}, "T"),
                         ({"ld_p": 99}, "ld_p"), ({"ld": 99}, "ld must"), ({"max_iv": -1}, "max_iv"), ({"p": None}, "d_probs"),
                         ({"cn": None}, "d_iv_counts"), ({"w": None}, "d_ws"), ({"w": C.c_void_p(0x1008)}, "d_ws"), ({"iv": None}, "d_iv "),
                         ({"nw": ws - 1}, f"need {ws} bytes"), ({"nw": 0}, f"need {ws} bytes")):
            assert call(**kw) == E_ARG and word in err(), kw
        assert call(B=1 << 22, T=1 << 20, ld_p=1 << 20, ld=1 << 20, nw=1 << 62) == E_ARG and "2^31" in err()   # more workgroups than a grid holds
        assert lib.uvad_binarize(None, fake, 100, 4, 100, None, C.byref(good), fake, 100, fake, 8, fake, fake, ws, None) == E_ARG
    finally:
        lib.uvad_destroy(ctx)


def test_host_configuration_refuses_bad_values(built):
    from uvad_amd.postprocess import binarize_config
    from uvad_amd.scripts import BINARIZE_DEFAULTS, _binarize_frames
    assert set(BINARIZE_DEFAULTS) == set(binarize_config.__code__.co_varnames[:6])
    assert _binarize_frames({"onset": 0.7, "offset": 0.4, "min_duration_on": 0.25, "pad_offset": 0.1}, False, 0.01) == \
        {"onset": 0.7, "offset": 0.4, "min_on": 25, "min_off": 0, "pad_on": 0, "pad_off": 10}
    assert _binarize_frames({"min_duration_on": 0.25, "pad_offset": 0.1}, True, 0.01) == \
        {"onset": 0.5, "offset": 0.5, "min_on": 15, "min_off": 0, "pad_on": 0, "pad_off": 6}      # 270-sample frames
    with pytest.raises(ValueError, match="unknown binarize option"):
        _binarize_frames({"onset": 0.5, "median": 49}, False, 0.01)
