"""CPU checks of the variable-length batch entries (uvad_*_lens, include/uvad.h): declared in the header, in the ctypes table and exported
by the library, ABI still 5; the lens instantiations of the kernels keep their resources (no scratch, the memory discipline of the
kernels they sit beside); and predict_vad's ragged batch packing (a pure host function) keeps the padded size within max_duration."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
NAMES = ["uvad_classify_lens", "uvad_forward_lens", "uvad_forward_lens_i16", "uvad_fbank_lens", "uvad_fbank_lens_i16",
         "uvad_median_filter_lens", "uvad_label_runs_lens"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_lens_entries_in_header_binding_and_export_list(built):
    src = _header()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in built.SIGNATURES, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    exported = set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert set(NAMES) <= exported
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", src) and built.ABI_VERSION == 5
    lib = built.load()
    assert lib.uvad_abi_version() == 5
    # the lengths follow the dense call's (B, T) / (B, S): int32 frames, int64 samples, both device pointers
    assert len(built.SIGNATURES["uvad_classify_lens"][1]) == len(built.SIGNATURES["uvad_classify"][1]) + 1
    assert len(built.SIGNATURES["uvad_forward_lens"][1]) == len(built.SIGNATURES["uvad_forward"][1]) + 1
    assert re.search(r"uvad_classify_lens\([^)]*int T, const int32_t \*d_lens", src)
    assert re.search(r"uvad_forward_lens\([^)]*int64_t S, const int64_t \*d_nsamp", src)


def test_lens_refusals_without_a_gpu_need_no_context(built):
    """A NULL context is UVAD_E_ARG before anything touches the device (the refusals with a context are GPU tests)."""
    lib = built.load()
    assert lib.uvad_classify_lens(None, None, 1, 1, None, None, None, None, 0, None) == -1
    assert lib.uvad_forward_lens(None, None, 1, 1, None, None, None, None, 0, None) == -1
    assert lib.uvad_median_filter_lens(None, None, 1, 1, None, 1, None, None) == -1
    assert lib.uvad_label_runs_lens(None, None, 1, 1, None, 1, None, None, None) == -1


def _isa(name):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    per = re.search(rf"^FLAGS_{name} := (.*)$", mk, re.M)
    per = [f for f in (per.group(1).split() if per else []) if not f.startswith("$(")]
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *flags, *per, "--cuda-device-only", "-S",
                          os.path.join(CSRC, name + ".hip"), "-o", "-"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def _kernels(isa):
    """{mangled name: (instructions, the listing up to the next kernel)} of every kernel in an -S listing."""
    out = {}
    labels = list(re.finditer(r"^(_Z\w+):", isa, re.M))
    for i, m in enumerate(labels):
        seg = isa[m.end():labels[i + 1].start() if i + 1 < len(labels) else len(isa)]
        out[m.group(1)] = (seg.split(".Lfunc_end")[0], seg)
    return out


@pytest.mark.parametrize("src,pat,n", [("lstm", r"lstm_rec\w*kernelI.*Lb1EEEv", 12), ("fbank", r"fbank_kernelI.*Lb1EEEv", 4)])
def test_lens_recurrence_and_feature_kernels_have_no_scratch(src, pat, n):
    ks = {k: v for k, v in _kernels(_isa(src)).items() if re.search(pat, k)}
    assert len(ks) == n, sorted(ks)
    for k, (body, meta) in ks.items():
        assert re.search(r"ScratchSize: 0\b", meta), k
        assert not re.search(r"^\s+scratch_", body, re.M), k


def test_lens_feature_kernel_keeps_the_32_bit_lds_forms():
    """tests/test_abi.py scans the fbank.hip listing from the first kernel on; the lens instantiations are checked by name here."""
    for k, (body, _) in _kernels(_isa("fbank")).items():
        if "fbank_kernel" not in k:
            continue
        lds = re.findall(r"^\s+(ds_[a-z0-9_]+)", body, re.M)
        assert lds, k
        assert not {op for op in lds if re.search(r"_b64$|_b96$", op)}, k
        assert not re.search(r"^\s+flat_(load|store|atomic)", body, re.M), k


def test_lens_post_processing_kernels_use_global_memory_only():
    """lens_fill / median_lens / runs_lens (head.hip) and the feature mask (gemm_f16p.hip) run beside the classifier's MFMA kernels:
    no LDS, no FLAT, no scratch, as the window-stream kernels."""
    found = 0
    for src, names in (("head", ("lens_fill_kernel", "median_lens_kernel", "runs_lens_kernel")), ("gemm_f16p", ("mask_features_kernel",))):
        for k, (body, meta) in _kernels(_isa(src)).items():
            if not any(n in k for n in names):
                continue
            found += 1
            assert not re.search(r"^\s+(flat|scratch)_", body, re.M), k
            assert not re.search(r"^\s+ds_", body, re.M), k
            assert re.search(r"ScratchSize: 0\b", meta), k
    assert found == 4


def test_ragged_packing_respects_max_duration_and_covers_every_recording_once():
    import random
    from uvad_amd.scripts import pack_ragged_batches
    rng = random.Random(5)
    for trial in range(50):
        lengths = [rng.randint(1, 2_000_000) for _ in range(rng.randint(1, 60))]
        cap = rng.choice([1_000_000, 6_400_000, 40_000_000])
        batches = pack_ragged_batches(lengths, cap)
        flat = [i for b in batches for i in b]
        assert sorted(flat) == list(range(len(lengths)))
        # sorted by length, longest first (ties by index): consecutive rows of one batch have close lengths
        assert flat == sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
        for b in batches:
            padded = len(b) * max(lengths[i] for i in b)
            assert padded <= cap or len(b) == 1, (trial, b)
        # greedy: no batch could have taken the next one's first row
        for b, nxt in zip(batches, batches[1:]):
            assert (len(b) + 1) * lengths[b[0]] > cap
    assert pack_ragged_batches([], 10) == []
    assert pack_ragged_batches([5, 30, 10], 30) == [[1], [2, 0]]
    assert pack_ragged_batches([5, 30, 10], 60) == [[1, 2], [0]]


def test_ragged_batches_is_off_by_default():
    from config.config import load_config
    assert load_config().ragged_batches is False


def test_pyannet_refuses_lengths_and_says_why():
    import torch
    import uvad_amd
    m = uvad_amd.PyanNet()
    with pytest.raises(NotImplementedError, match="instance norm"):
        m.forward(torch.zeros(1, 1, 16000), lengths=[16000])
    with pytest.raises(NotImplementedError, match="instance norm"):
        m.forward_logits(torch.zeros(1, 16000), lengths=[16000])
