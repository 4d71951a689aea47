"""CPU checks of the speech-cut entry points (uvad_cuts_*, include/uvad.h): declared in the header, bound in the ctypes table and
exported; the two records; the bounds; and every refusal, all of which are made before the library touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_cuts_max_per_row", "uvad_cuts_max_samples", "uvad_cuts_ws_bytes", "uvad_cuts_table", "uvad_cuts_gather"]
E_ARG = -1
SAMPLES, FRAMES = 0, 1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _cfg(built, pad=10, max_len=1000, min_len=10, hop=160, lead=0, tail=240):
    return built.CutsCfg(pad, max_len, min_len, hop, lead, tail)


def test_cuts_entries_in_header_binding_and_export_list(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_cuts_ws_bytes"][0] is C.c_size_t and built.SIGNATURES["uvad_cuts_max_samples"][0] is C.c_int64
    assert len(built.SIGNATURES["uvad_cuts_table"][1]) == 16 and len(built.SIGNATURES["uvad_cuts_gather"][1]) == 12
    assert built.load().uvad_abi_version() == built.ABI_VERSION == 5
    assert int(re.search(r"#define UVAD_ABI_VERSION (\d+)", src).group(1)) == 5
    assert int(re.search(r"#define UVAD_CUTS_SAMPLES (\d+)", src).group(1)) == built.CUTS_SAMPLES == SAMPLES
    assert int(re.search(r"#define UVAD_CUTS_FRAMES (\d+)", src).group(1)) == built.CUTS_FRAMES == FRAMES
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bcuts\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "cuts.hip")).read()
    for k in ("cuts_rows_kernel", "cuts_scan_kernel", "cuts_write_kernel", "cuts_gather_kernel"):
        assert k in kernel
    assert "asm" not in kernel and "atomic" not in re.sub(r"//.*", "", kernel)      # no inline assembly; no atomics in the code
    assert "predict.py:638-647" in open(os.path.join(ROOT, "include", "uvad.h")).read()


def test_records_match_the_header(built):
    src = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} uvad_cuts_cfg;", src).group(1), flags=re.S)
    fields = re.findall(r"\bint\s+(\w+);", body)
    assert fields == ["pad", "max_len", "min_len", "hop", "lead", "tail"] == [f[0] for f in built.CutsCfg._fields_]
    assert all(f[1] is C.c_int for f in built.CutsCfg._fields_) and C.sizeof(built.CutsCfg) == 24
    body = re.search(r"typedef struct \{([^}]*)\} uvad_cut;", src).group(1)
    assert re.findall(r"\b(\w+)[,;]", body) == ["row", "index", "first_frame", "n_frames", "first_sample", "n_samples"] == [f[0] for f in built.Cut._fields_]
    assert C.sizeof(built.Cut) == 32 and built.Cut.first_sample.offset == 16 and built.Cut.n_samples.offset == 24
    import cuts_ref
    assert cuts_ref.CUT_DTYPE.itemsize == 32 and [cuts_ref.CUT_DTYPE.fields[n][1] for n in cuts_ref.CUT_DTYPE.names] == [0, 4, 8, 12, 16, 24]


BAD_CFGS = [({"pad": -1}, "pad"), ({"pad": (1 << 20) + 1}, "pad"), ({"max_len": -1}, "max_len"), ({"max_len": (1 << 24) + 1}, "max_len"),
            ({"min_len": -1}, "min_len"), ({"max_len": 5, "min_len": 5}, "min_len"), ({"max_len": 5, "min_len": 9}, "min_len"),
            ({"hop": 0}, "hop"), ({"hop": -3}, "hop"), ({"lead": -1}, "lead"), ({"tail": -1}, "tail")]


def test_bounds_at_known_values(built):
    lib = built.load()
    q = _cfg(built)
    assert lib.uvad_cuts_max_per_row(C.byref(q), 1000) == 500 + 1 and lib.uvad_cuts_max_per_row(C.byref(q), 360000) == 180000 + 360
    assert lib.uvad_cuts_max_per_row(C.byref(q), 999) == 500 + 0 and lib.uvad_cuts_max_per_row(C.byref(q), 1) == 1
    assert lib.uvad_cuts_max_samples(C.byref(q), 57600000) == 1000 * 160 + 240 and lib.uvad_cuts_max_samples(C.byref(q), 1000) == 1000
    q0 = _cfg(built, max_len=0, min_len=0)
    assert lib.uvad_cuts_max_per_row(C.byref(q0), 9) == 5 and lib.uvad_cuts_max_samples(C.byref(q0), 123457) == 123457
    q1 = _cfg(built, pad=0, max_len=1, min_len=0, hop=270, lead=33, tail=721)
    assert lib.uvad_cuts_max_per_row(C.byref(q1), 9) == 5 + 9 and lib.uvad_cuts_max_samples(C.byref(q1), 1 << 40) == 270 + 33 + 721
    assert lib.uvad_cuts_max_per_row(C.byref(_cfg(built, pad=1 << 20, max_len=1 << 24, min_len=(1 << 24) - 1)), 1 << 30) == (1 << 29) + 64
    assert lib.uvad_cuts_max_per_row(None, 10) == 0 and lib.uvad_cuts_max_samples(None, 10) == 0
    assert lib.uvad_cuts_max_per_row(C.byref(q), 0) == 0 and lib.uvad_cuts_max_per_row(C.byref(q), (1 << 30) + 1) == 0
    assert lib.uvad_cuts_max_samples(C.byref(q), -1) == 0 and lib.uvad_cuts_max_samples(C.byref(q), 0) == 0
    for kw, _ in BAD_CFGS:
        bad = _cfg(built, **kw)
        assert lib.uvad_cuts_max_per_row(C.byref(bad), 100) == 0 and lib.uvad_cuts_max_samples(C.byref(bad), 100) == 0, kw


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    try:
        assert [lib.uvad_cuts_ws_bytes(ctx, B, T) for B, T in ((1, 1), (2, 9), (3, 1000), (1030, 9))] == \
            [16 + 16, 16 + 2 * 5 * 16, 32 + 3 * 500 * 16, 8240 + 1030 * 5 * 16]
        assert lib.uvad_cuts_ws_bytes(ctx, 0, 10) == 0 and lib.uvad_cuts_ws_bytes(ctx, 1, 0) == 0 and lib.uvad_cuts_ws_bytes(None, 1, 1) == 0
        assert lib.uvad_cuts_ws_bytes(ctx, 1, (1 << 30) + 1) == 0
        ws = lib.uvad_cuts_ws_bytes(ctx, 4, 100)
        good = _cfg(built)

        def table(lab=fake, ld=100, B=4, T=100, S=16240, q=good, tab=fake, max_cuts=8, first=fake, total=fake, w=fake, nw=ws):
            return lib.uvad_cuts_table(ctx, lab, ld, B, T, None, None, S, C.byref(q) if q is not None else None, tab, max_cuts, first, total, w, nw, None)
        for kw, word in BAD_CFGS:
            assert table(q=_cfg(built, **kw)) == E_ARG and word in err(), kw
        assert table(q=None) == E_ARG and "cfg" in err()
        for kw, word in (({"B": 0}, "B"), ({"T": 0}, "T"), ({"T": (1 << 30) + 1, "ld": (1 << 30) + 1}, "T"), ({"ld": 99}, "ld"), ({"S": -1}, "S"),
                         ({"max_cuts": -1}, "max_cuts"), ({"lab": None}, "d_labels"), ({"first": None}, "d_row_first"), ({"total": None}, "d_total"),
                         ({"w": None}, "d_ws"), ({"tab": None}, "d_table"), ({"nw": ws - 1}, f"need {ws} bytes")):
            assert table(**kw) == E_ARG and word in err(), kw
        assert table(B=1 << 22, T=1 << 20, ld=1 << 20, nw=1 << 62) == E_ARG and "2^31" in err()      # more cuts than d_total can count

        def gather(src=fake, stride=16240, unit=2, which=SAMPLES, tab=fake, total=fake, max_cuts=8, out=fake, ld_out=1000, out_len=fake):
            return lib.uvad_cuts_gather(ctx, src, stride, unit, which, tab, total, max_cuts, out, ld_out, out_len, None)
        for kw, word in (({"unit": 1}, "unit_bytes"), ({"unit": 3}, "unit_bytes"), ({"unit": 8}, "unit_bytes"), ({"unit": 0}, "unit_bytes"),
                         ({"which": FRAMES, "unit": 2}, "unit_bytes"), ({"which": FRAMES, "unit": 6}, "unit_bytes"),
                         ({"which": FRAMES, "unit": 4100}, "unit_bytes"), ({"which": FRAMES, "unit": 0}, "unit_bytes"),
                         ({"which": 2}, "which"), ({"which": -1}, "which"), ({"ld_out": 0}, "ld_out"), ({"ld_out": -5}, "ld_out"),
                         ({"ld_out": 1 << 31}, "ld_out"), ({"stride": -1}, "row_stride"), ({"max_cuts": -1}, "max_cuts"),
                         ({"src": None}, "d_src"), ({"tab": None}, "d_table"), ({"total": None}, "d_total"), ({"out": None}, "d_out"),
                         ({"out_len": None}, "d_out_len")):
            assert gather(**kw) == E_ARG and word in err(), kw
        assert lib.uvad_cuts_table(None, fake, 100, 4, 100, None, None, 0, C.byref(good), fake, 8, fake, fake, fake, ws, None) == E_ARG
        assert lib.uvad_cuts_gather(None, fake, 1, 2, SAMPLES, fake, fake, 1, fake, 1, fake, None) == E_ARG
    finally:
        lib.uvad_destroy(ctx)


def test_host_split_refuses_bad_lengths():
    from uvad_amd.postprocess import cuts_config, split_runs
    for bad in ((-1, 0), (5, 5), (5, -1), (0, -1)):
        with pytest.raises(ValueError):
            split_runs([(0, 10)], *bad)
    assert cuts_config(0.1, True, 10.0, 0.1) == {"pad": 10, "max_len": 1000, "min_len": 10, "hop": 160, "lead": 0, "tail": 240}
    assert cuts_config(0.25, False, frame_shift=270 / 16000, hop=270, tail=721) == {"pad": 15, "max_len": 0, "min_len": 0, "hop": 270, "lead": 0, "tail": 721}
