"""CPU checks of the cut-supervision join's entry points (uvad_cuts_join*, include/uvad.h): declared in the header, bound in the ctypes
table and exported; the constants; the kernel file's conventions; the workspace size; and every refusal, all of which are made before
the library touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_cuts_join_ws_bytes", "uvad_cuts_join"]
E_ARG = -1
OVERLAP, INSIDE = 0, 1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_join_entries_in_header_binding_and_export_list(built):
    text = open(os.path.join(ROOT, "include", "uvad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_cuts_join_ws_bytes"][0] is C.c_size_t and built.SIGNATURES["uvad_cuts_join"][0] is C.c_int
    assert len(built.SIGNATURES["uvad_cuts_join_ws_bytes"][1]) == 4 and len(built.SIGNATURES["uvad_cuts_join"][1]) == 18
    assert built.load().uvad_abi_version() == built.ABI_VERSION == 5                    # adding symbols does not move it
    assert int(re.search(r"#define UVAD_ABI_VERSION (\d+)", src).group(1)) == 5
    assert int(re.search(r"#define UVAD_JOIN_OVERLAP\s+(\d+)", src).group(1)) == built.JOIN_OVERLAP == OVERLAP
    assert int(re.search(r"#define UVAD_JOIN_INSIDE\s+(\d+)", src).group(1)) == built.JOIN_INSIDE == INSIDE
    assert int(re.search(r"#define UVAD_JOIN_AUDIT_WORDS\s+(\d+)", src).group(1)) == built.JOIN_AUDIT_WORDS == 8
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bjoin\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "join.hip")).read()
    for k in ("join_items_kernel", "join_count_kernel", "join_scan_kernel", "join_write_kernel"):
        assert k in kernel
    assert "asm" not in kernel and "atomic" not in re.sub(r"//.*", "", kernel)      # no inline assembly; no atomics in the code (cuts.hip's convention)
    for cite in ("predict.py:515-520", ":541", ":549-572", ":597-611"):
        assert cite in text, cite


def test_host_names_follow_the_header(built):
    from uvad_amd.postprocess import JOIN_REPORT_NAMES
    from uvad_amd.runtime import VadRuntime
    assert VadRuntime.JOIN_MODES == {"overlap": OVERLAP, "inside": INSIDE}
    names = dict(VadRuntime.JOIN_AUDIT_NAMES)
    assert sorted(names.values()) == list(range(8))
    assert [names[n] for n in JOIN_REPORT_NAMES] == [0, 2, 3, 4, 5, 6, 7] and names["New cuts"] == 1


def test_ws_bytes_at_known_values(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))
    try:
        ws = lambda B, max_iv, max_cuts: lib.uvad_cuts_join_ws_bytes(ctx, B, max_iv, max_cuts)
        # one int32 per cut rounded up to 16 bytes, then max_cuts + 1 int32 rounded up to 16 bytes; B and max_iv only have to be valid
        assert [ws(1, 0, 0), ws(1, 5, 1), ws(4, 9, 3), ws(4, 9, 4), ws(1030, 64, 8), ws(2, 10000, 180360)] == \
            [0 + 16, 16 + 16, 16 + 16, 16 + 32, 32 + 48, 721440 + 721456]
        assert ws(7, 100, 64) == ws(1, 0, 64) == 256 + 272
        assert ws(0, 1, 1) == 0 and ws(-1, 1, 1) == 0 and ws(1, -1, 1) == 0 and ws(1, 1, -1) == 0
        assert lib.uvad_cuts_join_ws_bytes(None, 1, 1, 1) == 0
        assert ws(1, 1 << 16, 1 << 15) == 0 and ws(1, 46341, 46341) == 0                 # max_cuts x max_iv above 2^31 - 1
        assert ws(1, 46340, 46341) > 0 and ws(1, (1 << 31) - 1, 1) == 16 + 16
    finally:
        lib.uvad_destroy(ctx)


def test_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    try:
        need = lib.uvad_cuts_join_ws_bytes(ctx, 4, 10, 8)

        def join(tab=fake, first=fake, total=fake, max_cuts=8, B=4, iv=fake, counts=fake, max_iv=10, mode=OVERLAP, pfirst=fake, pairs=fake,
                 max_pairs=16, item_cuts=fake, audit=fake, w=fake, nw=need):
            return lib.uvad_cuts_join(ctx, tab, first, total, max_cuts, B, iv, counts, max_iv, mode, pfirst, pairs, max_pairs, item_cuts, audit, w, nw, None)
        for kw, word in (({"B": 0}, "B"), ({"B": -2}, "B"), ({"max_iv": -1}, "max_iv"), ({"max_cuts": -1}, "max_cuts"), ({"max_pairs": -1}, "max_pairs"),
                         ({"mode": 2}, "mode"), ({"mode": -1}, "mode"), ({"first": None}, "d_row_first"), ({"total": None}, "d_total"),
                         ({"counts": None}, "d_iv_counts"), ({"pfirst": None}, "d_pair_first"), ({"audit": None}, "d_audit"), ({"w": None}, "d_ws"),
                         ({"tab": None}, "d_table"), ({"iv": None}, "d_iv"), ({"pairs": None}, "d_pairs"), ({"nw": need - 1}, f"need {need} bytes"),
                         ({"nw": 0}, f"need {need} bytes")):
            assert join(**kw) == E_ARG and word in err(), kw
        assert join(iv=None) == E_ARG and "d_iv is NULL" in err()                      # not d_iv_counts
        assert join(max_cuts=1 << 16, max_iv=1 << 15, nw=1 << 62) == E_ARG and "2^31" in err()      # more pairs than d_pair_first can count
        assert join(max_cuts=46341, max_iv=46341, nw=1 << 62) == E_ARG and "2^31" in err()
        assert lib.uvad_cuts_join(None, fake, fake, fake, 8, 4, fake, fake, 10, OVERLAP, fake, fake, 16, fake, fake, fake, need, None) == E_ARG
    finally:
        lib.uvad_destroy(ctx)
