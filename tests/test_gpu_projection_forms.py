"""The weight-stationary projection (csrc/gemm_f16p_ws.hip) at every column-tile count and in every K instantiation, against float64.

gemm_f16p_ws_kernel has eight instantiations (K / 16 in {4, 6, 8, 16} x three or four products) and three quantities that depend on the
number of 128-column tiles nt = 4 H D / 128 (1 .. 8): the grid (CUs / (8 nt) * (8 nt) workgroups: 240 at nt = 3, 5, 6 and 224 at nt = 7
on 256 CUs), the tile queue ((bid >> 3) % nt and one counter per (group, column tile)) and the store path.  The library takes the kernel
only for launches with ceil(M / 128) * nt >= 2 * CUs, so a small test never reaches it.  Here every case computes its batch from that
rule (cell_ref.ws_*) and the device's CU count, asserts that the rule admits it, and reads the gate matrix through the transparent cell
of tests/cell_ref.py: h = tanh(tanh(z)) against the float64 product under the derived bound, in the four GEMM modes.

  * the gate workspace persists between calls, so every checked call follows a call on the NEGATED features (tanh is odd: every gate
    differs wherever z != 0); a row tile the checked call does not write shows as an error of 2 |h|, thousands of bounds
  * f16p (weight-stationary) and f16p_stream (tile-streaming) must agree bit for bit, and three runs of f16p must (the queue hands the
    row tiles out in another order every run)
The operand preconditions, the rule's helpers and head_reference's slope factor are checked without a GPU (unmarked tests).
"""
import numpy as np
import pytest
import torch

import cell_ref as cr

gpu = pytest.mark.gpu

T_WS = 255                        # odd: with B = 1 (mod 4) every case ends in a partial 4-sequence tile and a partial 128-row tile
MODES = ("f16p", "f16p_stream", "f16p3", "f32")
# name: (F, hidden, bidirectional, nt): each K = F in whole 32s appears with two nt, each nt once
CASES = {
    "k64_nt1": (64, 32, False, 1),
    "k128_nt2": (128, 32, True, 2),
    "k96_nt3": (80, 96, False, 3),
    "k96_nt4": (80, 64, True, 4),
    "k128_nt5": (128, 160, False, 5),
    "k256_nt6": (256, 96, True, 6),
    "k64_nt7": (64, 224, False, 7),
    "k256_nt8": (256, 256, False, 8),
}


def _operands(case, cus):
    """-> (B, K, x, w, ref (B, T, H D) float64, R likewise, z, tiny share of R)."""
    F, H, bidir, nt = CASES[case]
    B = cr.ws_batch(nt, T_WS, cus)
    x, w = cr.projection_operands(F, B, T_WS, seed=400 + nt, H=H)
    z, R = cr.product_reference(x, w)
    tiny = np.abs(x[..., :6].astype(np.float64)) @ np.abs(w[:, :6].astype(np.float64)).T
    share = float(np.median(tiny / R))
    if bidir:                                     # the backward direction holds the same rows in reverse order (projection_state_dict)
        z, R = np.concatenate([z, z[..., ::-1]], -1), np.concatenate([R, R[..., ::-1]], -1)
    return B, cr.ws_padded_k(F), x, w, np.tanh(np.tanh(z)), R, z, share


def _assert_rule_admits(case, B, K, cus):
    F, H, bidir, nt = CASES[case]
    rows = cr.ws_rows(B, T_WS)
    assert cr.ws_nt(H, 2 if bidir else 1) == nt and K in cr.WS_K, (case, K)
    assert B % 4 == 1 and rows % 128 != 0, (case, B, rows)
    assert cr.ws_selected(rows, nt, K, cus), f"{case}: {B} x {T_WS} no longer reaches the weight-stationary kernel on {cus} CUs"
    assert rows >= 1.05 * cr.ws_min_rows(nt, cus) > rows - 4 * T_WS, (case, rows, cr.ws_min_rows(nt, cus))


# ------------------------------------------------------------------------------------------------ CPU: the rule, the operands, the head bound
def test_launch_size_rule_on_hand_worked_examples():
    # 33 x 256 at nt = 8 (H = 128, two directions): 36 x 256 = 9216 rows = 72 row tiles, 72 x 8 = 576 >= 512
    assert cr.ws_rows(33, 256) == 9216 and cr.ws_nt(128, 2) == 8 and cr.ws_selected(9216, 8, 64, 256)
    assert not cr.ws_selected(9216, 8, 64, 304) and not cr.ws_selected(9216, 8, 192, 256) and not cr.ws_selected(9216, 9, 64, 256)
    # 61 x 509 at nt = 4 (H = 64, two directions): 64 x 509 = 32576 rows = 255 row tiles; whole: 1020 >= 512; in two chunks 127 x 4 = 508 < 512
    assert cr.ws_rows(61, 509) == 32576 and cr.ws_selected(32576, 4, 128, 256)
    assert cr.ws_chunks_used(32576, 4, 2, 256) == 1 and cr.ws_chunks_used(32576, 4, 8, 256) == 1
    # cfg 2 (256 x 1000, nt = 8): 2000 row tiles, eight chunks of 250 x 8 = 2000 >= 512
    assert [cr.ws_chunks_used(cr.ws_rows(256, 1000), 8, n, 256) for n in (2, 3, 7, 8)] == [2, 3, 7, 8]
    # 256 x 512 at nt = 2 (H = 64, one direction): 1024 row tiles; 256 x 2 = 512 at four chunks, 204 x 2 = 408 at five
    assert [cr.ws_chunks_used(cr.ws_rows(256, 512), 2, n, 256) for n in (2, 3, 7, 8)] == [2, 3, 4, 4]
    assert cr.ws_padded_k(60) == 64 and cr.ws_padded_k(80) == 96 and cr.ws_padded_k(128) == 128 and cr.ws_padded_k(192) == 192
    # the smallest admitted row counts and the batches 5 % above them: 256 CUs by hand, and the property on other chips
    assert [cr.ws_min_rows(nt, 256) for nt in (1, 3, 8)] == [511 * 128 + 1, 170 * 128 + 1, 63 * 128 + 1]
    assert [cr.ws_batch(nt, T_WS, 256) for nt in range(1, 9)] == [269, 133, 89, 65, 53, 45, 37, 33]
    for cus in (64, 104, 228, 256, 304):
        for case in CASES:
            nt = CASES[case][3]
            B = cr.ws_batch(nt, T_WS, cus)
            _assert_rule_admits(case, B, cr.ws_padded_k(CASES[case][0]), cus)
            assert not cr.ws_selected(cr.ws_min_rows(nt, cus) - 1, nt, 64, cus) and cr.ws_selected(cr.ws_min_rows(nt, cus), nt, 64, cus)


@pytest.mark.parametrize("case", list(CASES))
def test_operands_of_every_case_meet_their_preconditions(case):
    """|z| <= 0.25 (tanh(tanh(z)) passes an error of z on almost undiminished), R <= 4, and the columns whose hi plane is an f16
    subnormal carry a real share of R -- for the batch of a 256-CU chip; the GPU test asserts the same on what it draws."""
    B, K, x, w, ref, R, z, share = _operands(case, 256)
    _assert_rule_admits(case, B, K, 256)
    print(f"{case}: B {B}, K {K}, |z| <= {np.abs(z).max():.3f}, R <= {R.max():.3f}, median f16-subnormal share of R {share:.4f}")
    assert np.abs(z).max() <= 0.25 and R.max() <= 4.0 and share > 0.02
    assert (np.abs(x[..., :6]) < 2.0 ** -14).all() and (np.abs(x[..., :6]) >= 2.0 ** -24).all()


def test_projection_operands_keep_their_earlier_draws():
    """H = 128, F in {64, 80} (the callers in test_gpu_cell_edges.py): no octave shift, and H = 128 by default -- the same generator
    calls in the same order as before the builder took H; pinned by a digest of the draws."""
    import hashlib
    dig = hashlib.sha256()
    for F in (64, 80):
        x, w = cr.projection_operands(F, 5, 7, seed=100 + F)
        assert w.shape == (128, F) and x.shape == (5, 7, F)
        assert np.abs(w[:, 10:]).max() < 2.0 ** -7 and np.abs(w[:, 10:]).min() >= 2.0 ** -10
        dig.update(x.tobytes() + w.tobytes())
    assert dig.hexdigest() == EARLIER_DRAWS_SHA256
    for F, s in ((128, 1), (256, 2)):
        w = cr.projection_operands(F, 2, 3, seed=1, H=96)[1]
        assert w.shape == (96, F) and np.abs(w[:, 10:]).max() < 2.0 ** (-7 - s) and np.abs(w[:, 10:]).min() >= 2.0 ** (-10 - s)


EARLIER_DRAWS_SHA256 = "29d761bc4426afdd9f4e84e110452b253dbacc722e0c6bed3450ce58add2cecc"


def test_head_reference_is_unchanged_for_slopes_up_to_one_and_scales_beyond():
    rng = np.random.default_rng(3)
    hw = cr.head_weights(128, seed=5)
    y = cr.wide_range(rng, (3, 5, 128), -12, 0)

    def plain(slope, mode):          # the bound as it was written before the slope factor
        a, e = y.astype(np.float64), 0.0
        for wk, bk in (("linear.0.weight", "linear.0.bias"), ("linear.1.weight", "linear.1.bias"), ("classifier.weight", "classifier.bias")):
            W, b = hw[wk].astype(np.float64), hw[bk].astype(np.float64)
            z = a @ W.T + b
            R = np.abs(a) @ np.abs(W).T + np.abs(b)
            e = (e @ np.abs(W).T if np.ndim(e) else 0.0) + R * cr.product_rel(W.shape[1], mode)
            a = z if wk.startswith("classifier") else np.where(z >= 0, z, slope * z)
        return a[..., 0], e[..., 0]

    for mode in MODES:
        for slope in (0.01, -0.5, 0.0, 1.0, -1.0):
            (lg, bd), (lg0, bd0) = cr.head_reference(y, hw, slope, mode), plain(slope, mode)
            assert np.array_equal(lg, lg0) and np.array_equal(bd, bd0), (mode, slope)
        for slope in (1.5, -3.0):
            (lg, bd), (lg0, bd0) = cr.head_reference(y, hw, slope, mode), plain(slope, mode)
            assert np.array_equal(lg, lg0) and (bd > bd0).all() and (bd <= bd0 * slope * slope * (1 + 1e-12)).all(), (mode, slope)


# ------------------------------------------------------------------------------------------------ GPU
def _run(rt, x):
    rt.classify(x)
    y, _ = rt.taps(lin=False)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_weight_stationary_projection_against_float64_at_every_tile_count(case):
    import uvad_amd
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    F, H, bidir, nt = CASES[case]
    B, K, x, w, ref, R, z, share = _operands(case, cus)
    _assert_rule_admits(case, B, K, cus)
    assert np.abs(z).max() <= 0.25 and R.max() <= 4.0 and share > 0.02, (np.abs(z).max(), R.max(), share)
    m = uvad_amd.PyanNet2(lstm={"hidden_size": H, "num_layers": 1, "bidirectional": bidir}, linear={"num_layers": 0}, encoding_dim=F)
    m.build()
    m.load_state_dict(cr.projection_state_dict(w, bidirectional=bidir))
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    rt.set_recurrent_tile(4)
    xd = torch.from_numpy(x).to(dev)
    xn = torch.from_numpy(-x).to(dev)
    hs = {}

    def checked(xin, want, mode, what):
        h = _run(rt, xin)
        assert np.isfinite(h).all(), (case, mode, what)
        ratio = np.abs(h.astype(np.float64) - want) / cr.product_bound(R, K, mode)
        r = float(ratio.max())
        print(f"{case}: F {F}, K {K}, nt {nt}, B {B} x T {T_WS} on {cus} CUs, {mode}{what}: worst err / bound {r:.3f}")
        assert r <= 1.0, (case, mode, what, r, np.unravel_index(int(ratio.argmax()), ratio.shape))
        return h

    def same_bits(h, want, what):
        diff = _bits(h) != _bits(want)
        assert not diff.any(), (f"{case}: {what}: {int(diff.sum())} of {diff.size} values differ, by up to "
                                f"{float(np.abs(h.astype(np.float64) - want)[diff].max()):.2e}")

    for mode in MODES:
        rt.set_gemm_mode(mode)
        checked(xn, -ref, mode, ", negated features")       # (tanh is odd and R even in x: the same bound) -- the workspace now holds these gates
        hs[mode] = checked(xd, ref, mode, "")
    same_bits(hs["f16p"], hs["f16p_stream"], "weight-stationary against tile-streaming gates")
    rt.set_gemm_mode("f16p")
    for rep in (1, 2):                                      # with the first: three runs, the same bits
        _run(rt, xn)
        same_bits(_run(rt, xd), hs["f16p"], f"run {rep + 1} of f16p against the first")
