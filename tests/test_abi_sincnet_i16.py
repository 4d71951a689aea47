"""CPU checks of the int16 SincNet entries of the C ABI (uvad_sincnet_i16, uvad_forward_wav_i16): declared in include/uvad.h, in the
ctypes table, and the ABI version raised to 5 with them on both sides of the boundary."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uvad.h")).read(), flags=re.S)


def test_header_declares_both_int16_sincnet_entries():
    src = _header()
    assert re.search(r"int\s+uvad_sincnet_i16\s*\(\s*uvad_ctx\s*\*\s*,\s*const\s+int16_t\s*\*\s*d_wav\s*,\s*int\s+B\s*,\s*int64_t\s+S\s*,"
                     r"\s*float\s*\*\s*d_feats\s*,\s*void\s*\*\s*d_workspace\s*,\s*size_t\s+ws_bytes\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+uvad_forward_wav_i16\s*\(\s*uvad_ctx\s*\*\s*,\s*const\s+int16_t\s*\*\s*d_wav\s*,\s*int\s+B\s*,\s*int64_t\s+S\s*,"
                     r"\s*float\s*\*\s*d_logits\s*,\s*float\s*\*\s*d_probs\s*,\s*void\s*\*\s*d_workspace\s*,\s*size_t\s+ws_bytes\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", src)


def test_abi_version_is_5_in_header_and_binding():
    from uvad_amd import _lib
    m = re.search(r"#define\s+UVAD_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == 5 == _lib.ABI_VERSION


def test_binding_declares_both_int16_sincnet_entries_like_their_f32_twins():
    import ctypes as C
    from uvad_amd import _lib
    for name in ("uvad_sincnet", "uvad_forward_wav"):
        assert name + "_i16" in _lib.SIGNATURES
        assert _lib.SIGNATURES[name + "_i16"] == _lib.SIGNATURES[name]
    assert _lib.SIGNATURES["uvad_sincnet_i16"][0] is C.c_int
