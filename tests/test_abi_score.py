"""CPU checks of the scoring stage's entry points (uvad_score_*, uvad_intervals_to_labels, include/uvad.h): declared in the header, bound
in the ctypes table and exported; the configuration struct; the sizes; and the refusals that are made before the library touches a device."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_intervals_to_labels", "uvad_score_configure", "uvad_score_state_bytes", "uvad_score_ws_bytes", "uvad_score_reset",
         "uvad_score_step", "uvad_score_totals"]
E_ARG, E_STATE = -1, -3


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def _cfg(built, points=((0.5, 25),), collar=0, bins=256, segment=0, n_points=None):
    q = built.ScoreCfg()
    q.n_points = len(points) if n_points is None else n_points
    for m, (t, k) in enumerate(points):
        q.threshold[m], q.kernel[m] = t, k
    q.collar, q.bins, q.segment = collar, bins, segment
    return q


def test_score_entries_in_header_binding_and_export_list(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
        proto = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(proto.split(",")) == len(built.SIGNATURES[name][1]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert built.SIGNATURES["uvad_score_state_bytes"][0] is C.c_size_t and built.SIGNATURES["uvad_score_ws_bytes"][0] is C.c_size_t
    assert len(built.SIGNATURES["uvad_score_step"][1]) == 14 and len(built.SIGNATURES["uvad_intervals_to_labels"][1]) == 10
    assert built.load().uvad_abi_version() == built.ABI_VERSION
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bscore\.hip\b", mk, re.M)
    kernel = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "score.hip")).read()
    for k in ("score_step_kernel", "score_fold_kernel", "iv_labels_kernel"):
        assert k in kernel
    assert "asm" not in kernel and not re.search(r"atomicAdd\s*\(\s*(?:\(\s*)?(?:float|double)", kernel)


def test_cfg_struct_matches_the_header(built):
    src = open(os.path.join(ROOT, "include", "uvad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} uvad_score_cfg;", src).group(1), flags=re.S)
    fields = re.findall(r"\b(int|float)\s+(\w+)(\[\w+\])?;", body)
    assert [(t, n, bool(a)) for t, n, a in fields] == [("int", "n_points", False), ("float", "threshold", True), ("int", "kernel", True),
                                                       ("int", "collar", False), ("int", "bins", False), ("int", "segment", False)]
    assert [f[0] for f in built.ScoreCfg._fields_] == [n for _, n, _ in fields]
    assert int(re.search(r"#define UVAD_SCORE_MAX_POINTS (\d+)", src).group(1)) == built.SCORE_MAX_POINTS == 8
    assert int(re.search(r"#define UVAD_SCORE_TOTALS_WORDS (\d+)", src).group(1)) == built.SCORE_TOTALS_WORDS == 40 + 2 * 1024
    assert C.sizeof(built.ScoreCfg) == 4 * (1 + 8 + 8 + 3)


def test_sizes_and_configuration_refusals(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))      # no tables, weights or model are needed; without a GPU the context is still returned
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)                         # never dereferenced
    try:
        assert lib.uvad_score_state_bytes(ctx) == 0 and lib.uvad_score_ws_bytes(ctx, 4, 100) == 0          # not configured
        assert lib.uvad_score_reset(ctx, fake, 1 << 20, None) == E_STATE and "uvad_score_configure" in err()
        assert lib.uvad_score_step(ctx, fake, 100, fake, 100, 4, 100, None, fake, 1 << 20, None, fake, 1 << 20, None) == E_STATE
        bad = [(_cfg(built, n_points=0), "n_points"), (_cfg(built, n_points=9), "n_points"),
               (_cfg(built, [(0.5, 24)]), "kernel"), (_cfg(built, [(0.5, 0)]), "kernel"), (_cfg(built, [(0.5, 257)]), "kernel"),
               (_cfg(built, [(0.5, 25), (0.5, 2)]), "kernel"), (_cfg(built, [(math.nan, 25)]), "threshold"), (_cfg(built, [(math.inf, 1)]), "threshold"),
               (_cfg(built, collar=-1), "collar"), (_cfg(built, collar=1025), "collar"),
               (_cfg(built, bins=0), "bins"), (_cfg(built, bins=1), "bins"), (_cfg(built, bins=48), "bins"), (_cfg(built, bins=2048), "bins"),
               (_cfg(built, segment=-1), "segment"), (_cfg(built, segment=(1 << 14) + 1), "segment")]
        for q, word in bad:
            assert lib.uvad_score_configure(ctx, C.byref(q)) == E_ARG and word in err(), word
        assert lib.uvad_score_configure(ctx, None) == E_ARG
        assert lib.uvad_score_state_bytes(ctx) == 0                                                          # a refused configuration configures nothing
        assert lib.uvad_score_configure(ctx, C.byref(_cfg(built, [(0.5, 25), (0.3, 1), (0.5, 255)], 3, 1024, 64))) == 0
        state = lib.uvad_score_state_bytes(ctx)
        assert state == 256 + 8 * built.SCORE_TOTALS_WORDS
        w = [lib.uvad_score_ws_bytes(ctx, B, T) for B, T in ((1, 64), (1, 65), (7, 1031), (8, 1031))]
        assert w == [32 + 32 * 1, 32 + 32 * 2, 32 + 32 * 7 * 17, 32 + 32 * 8 * 17]
        assert lib.uvad_score_ws_bytes(ctx, 0, 10) == 0 and lib.uvad_score_ws_bytes(ctx, 1, 0) == 0 and lib.uvad_score_ws_bytes(None, 1, 1) == 0
        assert lib.uvad_score_configure(ctx, C.byref(_cfg(built))) == 0
        assert lib.uvad_score_ws_bytes(ctx, 256, 1000) == 32 + 32 * 256 and lib.uvad_score_ws_bytes(ctx, 1, 360000) == 32 + 32 * 176   # default segment 2048
    finally:
        lib.uvad_destroy(ctx)


def test_call_refusals_made_before_a_device_is_touched(built):
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)
    try:
        assert lib.uvad_score_configure(ctx, C.byref(_cfg(built, segment=64))) == 0
        state, ws = lib.uvad_score_state_bytes(ctx), lib.uvad_score_ws_bytes(ctx, 4, 100)
        assert lib.uvad_score_reset(ctx, None, state, None) == E_ARG
        assert lib.uvad_score_reset(ctx, fake, state - 1, None) == E_ARG and f"need {state} bytes" in err()
        step = lambda probs=fake, ld_p=100, gt=fake, ld_gt=100, B=4, T=100, st=fake, nst=state, w=fake, nw=ws: \
            lib.uvad_score_step(ctx, probs, ld_p, gt, ld_gt, B, T, None, st, nst, None, w, nw, None)
        for kw in ({"probs": None}, {"gt": None}, {"st": None}, {"w": None}, {"B": 0}, {"T": 0}, {"T": (1 << 30) + 1}, {"ld_p": 99}, {"ld_gt": 99},
                   {"nst": state - 1}, {"nw": ws - 1}):
            assert step(**kw) == E_ARG, kw
        assert "need" in err()
        assert step() == E_STATE and "uvad_score_reset" in err()            # arguments in order, but the state was never reset
        assert lib.uvad_score_totals(ctx, fake, state, fake, None) == E_STATE
        assert lib.uvad_score_totals(ctx, fake, state, None, None) == E_ARG and lib.uvad_score_totals(ctx, fake, state - 1, fake, None) == E_ARG
        iv = lambda ivp=fake, cn=fake, B=4, max_iv=3, T=100, ld=100, lab=fake: lib.uvad_intervals_to_labels(ctx, ivp, cn, B, max_iv, T, ld, None, lab, None)
        for kw in ({"ivp": None}, {"cn": None}, {"lab": None}, {"B": 0}, {"T": 0}, {"max_iv": -1}, {"ld": 99}):
            assert iv(**kw) == E_ARG, kw
    finally:
        lib.uvad_destroy(ctx)
