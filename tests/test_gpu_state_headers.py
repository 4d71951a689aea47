"""GPU tests (-m gpu) of what a reset leaves in the four device states that begin with a 256-byte header -- the live endpointers
(uvad_endpoint_*, uvad_endpoint_hyst_*) and the live speech gates (uvad_gate_*, uvad_gate_group_*) -- opened through VadRuntime with a
distinct, non-default value in every field: the header's 64 little-endian words one by one (the words the step kernels read by field
name), zeros in every other header word and in every byte of the slots that follow, and the same header after a step."""
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CUTS = dict(pad=2, max_len=9, hop=4, lead=3, tail=5)                        # min_len is 0 in every gate
GATE_SLOT, GROUP_SLOT = 64, 96                                              # bytes per slot / per group


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def lo_hi(v):
    return [v & 0xffffffff, v >> 32]


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def _endpoint(rt):
    ep = rt.endpoint_open(2, 8, kernel=7, pad=3, threshold=0.375)
    step = lambda: rt.endpoint_step(ep, torch.full((2, 8), 0.9, device=DEV), torch.tensor([8, 5], dtype=torch.int32, device=DEV), start=[0, 1])
    return ep["state"], [0x55564550, 2, 7, 3, bits(0.375)], ep["state"].numel() - 256, step


def _endpoint_hyst(rt):
    ep = rt.endpoint_hyst_open(2, 8, onset=0.625, offset=0.25, min_on=3, min_off=4, pad_on=5, pad_off=6)
    step = lambda: rt.endpoint_hyst_step(ep, torch.full((2, 8), 0.9, device=DEV), torch.tensor([8, 5], dtype=torch.int32, device=DEV), start=[0, 1])
    return ep["state"], [0x55564548, 2, bits(0.625), bits(0.25), 3, 4, 5, 6], ep["state"].numel() - 256, step


def _gate(rt):
    g = rt.gate_open(2, 6, 5, torch.int16, 2, history=37, **CUTS)
    ring = (37 * 2 + 15) // 16 * 16
    assert g["state"].numel() == 256 + 2 * (GATE_SLOT + ring)
    step = lambda: rt.gate_step(g, torch.ones((2, 6), dtype=torch.int16, device=DEV), torch.ones((2, 5), dtype=torch.uint8, device=DEV),
                                torch.tensor([3, 1], dtype=torch.int32, device=DEV), start=[0, 1])
    return g["state"], [0x55564754, 2, 2, 9, 0, 4, 3, 5, 2, 37] + lo_hi(ring), 2 * GATE_SLOT, step


def _gate_group(rt):
    fz = rt.fuse_open([[0, 1], [2, 3]])
    g = rt.gate_group_open(fz, 6, 5, torch.float32, 2, 3, history=41, best_history=11, **CUTS)
    ring, best = (41 * 4 + 15) // 16 * 16, 16
    assert g["state"].numel() == 256 + 2 * (GROUP_SLOT + best) + 4 * ring
    counts = torch.tensor([3, 1], dtype=torch.int32, device=DEV)
    step = lambda: rt.gate_group_step(g, torch.ones((4, 6), dtype=torch.float32, device=DEV), torch.zeros((2, 5), dtype=torch.uint8, device=DEV), counts,
                                      torch.ones((2, 5), dtype=torch.uint8, device=DEV), counts, start=[0, 1])
    return g["state"], [0x55564747, 2, 4, 2, 9, 0, 4, 3, 5, 4, 41, 11, 3, 0] + lo_hi(ring) + lo_hi(best), 2 * GROUP_SLOT, step


@pytest.mark.parametrize("which", [_endpoint, _endpoint_hyst, _gate, _gate_group], ids=["endpoint", "endpoint_hyst", "gate", "gate_group"])
def test_reset_writes_the_header_words_and_zero_slots(rt, which):
    state, words, slot_bytes, step = which(rt)
    torch.cuda.synchronize()
    raw = state.cpu().numpy()
    header = raw[:256].view("<u4")
    want = np.zeros(64, np.uint32)
    want[:len(words)] = words
    assert header.tolist() == want.tolist()
    assert slot_bytes > 0 and not raw[256:256 + slot_bytes].any()
    step()
    torch.cuda.synchronize()
    after = state.cpu().numpy()
    assert after[:256].tobytes() == raw[:256].tobytes()                     # a step reads the header and never writes it
    assert after[256:256 + slot_bytes].any()                                # ... and the step did run: both slots started a session
