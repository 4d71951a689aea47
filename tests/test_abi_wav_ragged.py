"""CPU checks of the variable-length entries of the waveform model (uvad_sincnet_lens[_i16], uvad_forward_wav_lens[_i16]): declared in
the header with d_nsamp right after S, in the ctypes table and exported, ABI still 5; a NULL context is refused before anything touches a
device; and the lens instantiations of the SincNet kernels (both forms of the conv stages, statistics, finalizers, output, geometry)
have no scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
NAMES = ["uvad_sincnet_lens", "uvad_sincnet_lens_i16", "uvad_forward_wav_lens", "uvad_forward_wav_lens_i16"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from uvad_amd import _lib
    return _lib


def test_wav_lens_entries_in_header_binding_and_export_list(built):
    src = _header()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf"{name}\([^)]*int64_t S, const int64_t \*d_nsamp", src), name
        assert name in built.SIGNATURES, name
        dense = name.replace("_lens", "")
        assert len(built.SIGNATURES[name][1]) == len(built.SIGNATURES[dense][1]) + 1, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    assert set(NAMES) <= set(re.findall(r" T (uvad_[a-z0-9_]+)", out))
    assert re.search(r"#define\s+UVAD_ABI_VERSION\s+5\b", src) and built.ABI_VERSION == 5
    assert built.load().uvad_abi_version() == 5


def test_wav_lens_null_context_is_refused(built):
    lib = built.load()
    assert lib.uvad_sincnet_lens(None, None, 1, 16000, None, None, None, 0, None) == -1
    assert lib.uvad_sincnet_lens_i16(None, None, 1, 16000, None, None, None, 0, None) == -1
    assert lib.uvad_forward_wav_lens(None, None, 1, 16000, None, None, None, None, 0, None) == -1
    assert lib.uvad_forward_wav_lens_i16(None, None, 1, 16000, None, None, None, None, 0, None) == -1


def _isa(name):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    per = re.search(rf"^FLAGS_{name} := (.*)$", mk, re.M)
    per = [f for f in (per.group(1).split() if per else []) if not f.startswith("$(")]
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *flags, *per, "--cuda-device-only", "-S",
                          os.path.join(CSRC, name + ".hip"), "-o", "-"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def _kernels(isa):
    out = {}
    labels = list(re.finditer(r"^(_Z\w+):", isa, re.M))
    for i, m in enumerate(labels):
        seg = isa[m.end():labels[i + 1].start() if i + 1 < len(labels) else len(isa)]
        out[m.group(1)] = (seg.split(".Lfunc_end")[0], seg)
    return out


# lens instantiations by mangled name: the conv kernels end their template list with LENS = true (Lb1EEE); the small kernels are
# templates on LENS alone (ILb1EE); the geometry kernel exists for lens calls only
@pytest.mark.parametrize("src,pat,n", [
    ("sincnet_f16p", r"sinc_conv_f16p_kernelI.*Lb1EEEv", 4),
    ("sincnet_f16p", r"(norm_finalize_f16p_kernel|sinc_out_f16p_kernel)ILb1EE", 2),
    ("sincnet", r"conv_pool_kernelI.*Lb1EEEv", 16),
    ("sincnet", r"(wav_stats_kernel|wav_stats_i16_kernel|norm_finalize_kernel|sinc_out_kernel)ILb1EE", 4),
    ("sincnet", r"sinc_row_geometry_kernel", 1),
])
def test_lens_sincnet_kernels_have_no_scratch(src, pat, n):
    ks = {k: v for k, v in _kernels(_isa(src)).items() if re.search(pat, k)}
    assert len(ks) == n, sorted(ks)
    for k, (body, meta) in ks.items():
        assert re.search(r"ScratchSize: 0\b", meta), k
        assert not re.search(r"^\s+scratch_", body, re.M), k
