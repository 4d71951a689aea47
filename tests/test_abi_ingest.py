"""CPU checks of the ingest stage (uvad_ingest*, include/uvad.h): the entries are declared, bound and exported; a library that lacks
one is a loud error by name; the tap design, the G.711 tables, the RIFF reader and the plan against the float64 restatement
(tests/ingest_ref.py); the refusals the library makes before it touches a device; the kernel's LDS instruction forms."""
import audioop
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ingest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uvad_ingest_configure", "uvad_ingest_set_taps", "uvad_ingest_out_len", "uvad_ingest_state_bytes", "uvad_ingest", "uvad_ingest_lens",
         "uvad_ingest_stream_reset", "uvad_ingest_stream_step"]
E_ARG, E_STATE, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4, -5
RATES = {8000: (2, 1, 7, 15), 48000: (1, 3, 19, 41), 32000: (1, 2, 13, 28), 24000: (2, 3, 10, 23)}   # rate: (up, down, width, K)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_ingest_entries_in_header_binding_and_export_list(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", src) and built.ABI_VERSION == 5      # append-only: the number stays
    for i, enc in enumerate(("F32", "I16", "ULAW", "ALAW")):
        assert re.search(rf"#define\s+UVAD_INGEST_{enc}\s+{i}\b", src)
    from uvad_amd.ingest import ENCODINGS, MAX_PHASES, MAX_TAPS
    assert ENCODINGS == {"f32": 0, "int16": 1, "ulaw": 2, "alaw": 3}
    assert re.search(rf"#define\s+UVAD_INGEST_MAX_PHASES\s+{MAX_PHASES}\b", src) and re.search(rf"#define\s+UVAD_INGEST_MAX_TAPS\s+{MAX_TAPS}\b", src)
    assert C.sizeof(built.IngestCfg) == 3 * 4
    mk = open(os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bingest\.hip\b", mk, re.M)


def test_a_library_without_an_ingest_symbol_is_a_loud_error_by_name(built):
    """The ABI number did not move, so an older libuvad.so passes the version check: binding must name what is missing."""
    class Fn:
        restype = argtypes = None

    class OldLib:                      # exports everything but the ingest stage
        def __getattr__(self, name):
            if name.startswith("uvad_ingest"):
                raise AttributeError(name)
            fn = Fn()
            object.__setattr__(self, name, fn)
            return fn

    with pytest.raises(RuntimeError, match=r"does not export uvad_ingest\w*: .*rebuild the library"):
        built.bind(OldLib())

    class Whole(OldLib):
        def __getattr__(self, name):
            fn = Fn()
            object.__setattr__(self, name, fn)
            return fn

    lib = built.bind(Whole())
    assert lib.uvad_ingest_stream_step.argtypes == built.SIGNATURES["uvad_ingest_stream_step"][1]


def test_resample_taps_shapes_widths_and_the_44100_refusal():
    from uvad_amd.ingest import resample_taps
    from uvad_amd import runtime
    assert runtime.resample_taps is resample_taps
    for rate, (up, down, width, K) in RATES.items():
        taps, u, d, w = resample_taps(rate)
        assert (u, d, w) == (up, down, width) and taps.shape == (up, K) and taps.dtype == np.float32
        want, nu, nd, nw = ref.taps_f64(rate)
        assert (nu, nd, nw) == (up, down, width)
        assert np.abs(taps.astype(np.float64) - want).max() <= 2.0 ** -24 * np.abs(want).max() * 1.01     # the f32 rounding of the f64 design
        sums = taps.astype(np.float64).sum(1)
        assert (sums > 0.99995).all() and (sums < 1.00095).all(), sums
    assert resample_taps(16000) == (None, 1, 1, 0)
    with pytest.raises(ValueError, match=r"160 phases x 475 taps.*limit of 8 phases x 64 taps"):
        resample_taps(44100)


def test_g711_tables_equal_audioop_on_all_256_codes():
    from uvad_amd.ingest import g711_table
    codes = bytes(range(256))
    assert g711_table("ulaw").tolist() == np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2").tolist()
    assert g711_table("alaw").tolist() == np.frombuffer(audioop.alaw2lin(codes, 2), "<i2").tolist()
    with pytest.raises(ValueError):
        g711_table("pcm")


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("tag,encoding", [(1, "int16"), (6, "alaw"), (7, "ulaw")])
def test_read_audio_round_trips_written_files(tmp_path, tag, encoding, channels):
    from uvad_amd.scripts import read_audio
    rng = np.random.default_rng(tag * 10 + channels)
    n = 1237                                                   # odd: the data chunk of an 8-bit mono file needs its pad byte
    raw = rng.integers(-32768, 32768, (n, channels)).astype(np.int16) if tag == 1 else rng.integers(0, 256, (n, channels)).astype(np.uint8)
    p = str(tmp_path / "a.wav")
    ref.write_wav(p, raw, tag, 8000 if tag != 1 else 44100)
    got, (enc, ch, rate) = read_audio(p)
    assert (enc, ch, rate) == (encoding, channels, 8000 if tag != 1 else 44100)
    assert got.dtype == raw.dtype and got.shape == raw.shape and (got == raw).all()
    ref.write_wav(p, rng.integers(0, 256, (16, 1)).astype(np.uint8), 2, 8000)        # ADPCM: not supported
    with pytest.raises(ValueError, match="format tag 2"):
        read_audio(p)
    open(p, "wb").write(b"RIFX" + b"\0" * 40)
    with pytest.raises(ValueError, match="not a RIFF/WAVE"):
        read_audio(p)


@pytest.mark.parametrize("rate", [8000, 24000, 32000, 48000])
def test_ingest_plan_lengths_and_delay_against_the_float64_helper(rate):
    from uvad_amd.ingest import ingest_plan, resample_taps
    rng = np.random.default_rng(rate)
    lengths = [0, 1, 2, 3] + rng.integers(0, 100000, 60).tolist()
    taps, up, down, width = resample_taps(rate)
    plan = ingest_plan(rate, lengths)
    assert (plan["up"], plan["down"], plan["width"], plan["taps_per_phase"]) == (up, down, width, taps.shape[1])
    assert plan["delay"] == ref.delay(up, down, width)
    assert plan["history"] == plan["delay"] // up * down + width
    for n, m in zip(lengths, plan["lengths"]):
        assert m == ref.out_len(n, up, down) and (m - 1) * down < n * up <= m * down or (n == 0 and m == 0)
        if n < 3000:
            assert len(ref.resample_f64(np.zeros(n), taps, up, down, width)) == m
    assert ingest_plan(rate, 17)["lengths"] == ref.out_len(17, up, down)
    assert ingest_plan(8000, 5)["delay"] == 14                  # 0.875 ms
    p16 = ingest_plan(16000, [0, 1, 7])
    assert (p16["delay"], p16["history"], p16["lengths"]) == (0, 0, [0, 1, 7])
    # the delay is the least whole number of output groups that keeps a step out of the future: group j of a stream reads input up to
    # (j - dj) down + K - 1 - width, and by the time its own down inputs have arrived the stream holds them up to j down + down - 1
    dj, reach = plan["delay"] // up, taps.shape[1] - 1 - width
    assert -dj * down + reach <= down - 1 < -(dj - 1) * down + reach


def test_sine_through_the_published_filter_on_the_cpu_helper():
    """Sanity on real content (not a gate on the kernel): a 1 kHz sine at 8 kHz through the f64 restatement against the analytic 16 kHz
    sine, away from the edges.  The error is a property of the published filter (its pass-band gain at 1 kHz), recorded in DESIGN.md."""
    taps, up, down, width = ref.taps_f64(8000)
    n = 4000
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / 8000.0)
    y = ref.resample_f64(x, taps, up, down, width)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 16000.0)
    err = np.abs(y - want)[100:-100].max()
    print(f"1 kHz sine, 8 -> 16 kHz, published filter, float64: max error away from the edges {err:.3e}")
    assert np.isfinite(err)            # recorded, not gated: it grades the published design, not this project's kernel


def test_the_library_refuses_with_named_messages(built):
    """Every refusal below is made before the library touches a device, so it reads the same here, where uvad_create itself has failed
    for want of a GPU (the context is still returned for uvad_last_error) -- and on a GPU machine, where it has succeeded."""
    lib = built.load()
    ctx = C.c_void_p()
    lib.uvad_create(0, None, None, C.byref(ctx))
    err = lambda: lib.uvad_last_error(ctx).decode()
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused first
    try:
        # before configure
        assert lib.uvad_ingest(ctx, fake, 1, 160, fake, None) == E_STATE and "uvad_ingest_configure first" in err()
        assert lib.uvad_ingest_stream_step(ctx, fake, None, 1, 160, fake, 1 << 20, fake, None) == E_STATE and "uvad_ingest_configure first" in err()
        taps = np.zeros((160, 475), np.float32)
        assert lib.uvad_ingest_set_taps(ctx, taps.ctypes.data, 160, 441, 17) == E_STATE
        assert lib.uvad_ingest_out_len(ctx, 100) == E_STATE and lib.uvad_ingest_state_bytes(ctx, 4) == 0
        # configure
        cfg = built.IngestCfg(7, 1, 8000)
        assert lib.uvad_ingest_configure(ctx, C.byref(cfg)) == E_ARG and "encoding" in err()
        cfg = built.IngestCfg(2, 9, 8000)
        assert lib.uvad_ingest_configure(ctx, C.byref(cfg)) == E_UNSUPPORTED and "at most 8" in err()
        # a table above the limits: 44.1 kHz needs 160 phases x 475 taps
        cfg = built.IngestCfg(1, 2, 44100)
        assert lib.uvad_ingest_configure(ctx, C.byref(cfg)) == 0
        assert lib.uvad_ingest_out_len(ctx, 441) == 160
        assert lib.uvad_ingest_set_taps(ctx, taps.ctypes.data, 160, 441, 17) == E_UNSUPPORTED
        assert "160 phases x 475 taps" in err() and "limit of 8 phases x 64 taps" in err()
        assert lib.uvad_ingest_set_taps(ctx, taps.ctypes.data, 2, 1, 7) == E_ARG and "needs 160 / 441" in err()
        assert lib.uvad_ingest(ctx, fake, 1, 441, fake, None) == E_STATE and "no resampler taps for 160 / 441" in err()
        assert lib.uvad_ingest_state_bytes(ctx, 4) == 0
        # 48 kHz: 1 / 3 -- chunk_in must be a multiple of down
        cfg = built.IngestCfg(2, 1, 48000)
        assert lib.uvad_ingest_configure(ctx, C.byref(cfg)) == 0
        assert lib.uvad_ingest_stream_step(ctx, fake, None, 4, 961, fake, 1 << 20, fake, None) == E_ARG
        assert "multiple of down = 3" in err()
        wide = np.zeros((1, 2 * 31 + 3), np.float32)           # 65 taps per phase
        assert lib.uvad_ingest_set_taps(ctx, wide.ctypes.data, 1, 3, 31) == E_UNSUPPORTED and "1 phases x 65 taps" in err()
        # 16 kHz: no table; a state that is too small
        cfg = built.IngestCfg(1, 2, 16000)
        assert lib.uvad_ingest_configure(ctx, C.byref(cfg)) == 0
        one = np.ones((1, 1), np.float32)
        assert lib.uvad_ingest_set_taps(ctx, one.ctypes.data, 1, 1, 0) == E_ARG and "takes no table" in err()
        need = lib.uvad_ingest_state_bytes(ctx, 4)
        assert need > 0
        assert lib.uvad_ingest_stream_step(ctx, fake, None, 4, 320, fake, need - 1, fake, None) == E_WORKSPACE
        assert f"need {need} bytes" in err()
        assert lib.uvad_ingest_stream_reset(ctx, fake, need - 1, 4, None) == E_WORKSPACE and f"need {need} bytes" in err()
        assert lib.uvad_ingest_stream_step(ctx, None, None, 4, 320, fake, need, fake, None) == E_ARG
        assert lib.uvad_ingest_lens(ctx, fake, 4, 320, None, fake, fake, None) == E_ARG
    finally:
        lib.uvad_destroy(ctx)


def test_ingest_kernel_lds_forms_and_no_scratch():
    """The ingest kernel runs beside the MFMA kernels of a served step: 32-bit LDS operations only (the forms that have run in flight
    without corruption, tests/test_abi.py), no FLAT access, no scratch; its outputs leave as 16-byte vector stores."""
    csrc = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S",
                          os.path.join(csrc, "ingest.hip"), "-o", "-"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    isa = out.stdout
    assert isa.count("ingest_kernel") >= 3
    lds = set(re.findall(r"^\s+(ds_[a-z0-9_]+)", isa, re.M))
    assert lds and lds <= {"ds_read_b32", "ds_write_b32", "ds_read2_b32", "ds_write2_b32", "ds_read2st64_b32", "ds_write2st64_b32"}, lds
    assert not re.search(r"^\s+(flat|scratch)_", isa, re.M)
    assert "global_store_dwordx4" in isa
    assert re.search(r"ScratchSize: 0", isa) and not re.search(r"ScratchSize: [1-9]", isa)
    assert "v_fma_f32" in isa or "v_fmac_f32" in isa
