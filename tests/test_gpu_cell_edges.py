"""Controlled-operand edge tests of the recurrent cell and the split-f16 products (reference and builders: tests/cell_ref.py).

  cell isolation   W_hh = 0 and 0/1 selection rows in W_ih make every gate pre-activation an exactly known number, and the LSTM tap
                   returns h as the kernel computed it: every recurrence form (H = 128 with 4 and 16 sequences per workgroup, H = 64,
                   the generic kernel at H = 32 and H = 96; dense and per-row lengths; GEMM modes f32 and f16p) against a float64 cell
                   on a grid with exact zeros, tiny values, the exponent clamp (87 .. 89) and values far beyond it, inside the bound
                   DERIVED from the contract of csrc/lstm.hip (cell_ref.lstm_reference), plus a 300-step case where |c| grows to 300
  containment      one NaN / +Inf in one sequence changes no bit of any other sequence in the kernels that share sequences inside
                   matrix-core tiles, is non-finite exactly where torch's CPU LSTM is, and leaves nothing behind in the workspace
  bottom of f16    the input projection on features whose hi plane is an f16 subnormal and on a weight matrix spanning 20 octaves,
                   read through a transparent cell, in every GEMM mode and both projection kernels (every column-tile count and K of
                   the weight-stationary one: tests/test_gpu_projection_forms.py)
  head             wide-range feed-forward / classifier weights against a float64 head on the tapped LSTM output: both input widths
                   of head_fused_kernel, row counts with more 64-row tiles than CUs, leaky_relu slopes from -0.5 to 1.5
The GPU tests carry the gpu mark one by one: the float32 restatement test runs without a GPU.
"""
import numpy as np
import pytest
import torch

import cell_ref as cr

gpu = pytest.mark.gpu

# name: (hidden, bidirectional, recurrent tile)
FORMS = {"h128_tile4": (128, True, 4), "h128_tile16": (128, True, 16), "h64": (64, True, 4), "h32_generic": (32, True, 4),
         "h96_uni_generic": (96, False, 4)}
B1, T1 = 21, 6                                                    # five full 4-tiles and a partial one; a full and a partial 16-tile
LENS1 = [6, 1, 0, 3, 5, 2, 6, 4, 0, 1, 6, 2, 5, 3, 6, 6, 1, 4, 2, 0, 5]
TWINS = [(20, 0), (17, 3), (9, 16)]                               # rows with identical features in different tiles


# ------------------------------------------------------------------------------------------------ CPU: the bound itself
def test_float32_restatement_of_both_cells_stays_below_half_the_bound():
    """lstm_cell and lstm_cell1 restated in float32 with a correctly rounded exp2 / reciprocal, 200 000 sequences of 6 steps on the
    grid: every value finite and no error above 0.5 of the derived bound (hardware exp2 / reciprocal at 1 ulp each then have room)."""
    N, T = 200000, 6
    pre = cr.grid_values((N, T, 4), seed=2024)
    ref, bound = cr.lstm_reference(pre.astype(np.float64).transpose(0, 1, 2)[None, :, :, :, None])
    ref, bound = ref[..., 0], bound[..., 0]
    for name, cell in (("lstm_cell", cr.cell_f32), ("lstm_cell1", cr.cell1_f32)):
        h = cr.run_cell_f32(cell, pre)
        assert np.isfinite(h).all(), name
        err = np.abs(h.astype(np.float64) - ref)
        ratio = float((err / bound).max())
        print(f"{name}: worst err / bound {ratio:.3f}, worst |err| {err.max() / cr.EPS:.2f} ulp(1)")
        assert ratio < 0.5, (name, ratio)
    # the NaN semantics the kernels have (pinned, not changed): fminf swallows a NaN in a sigmoid gate, tanh_f propagates it
    assert np.isfinite(cr.sigmoid_f32(np.float32("nan"))) and np.isnan(cr.tanh_f32(np.float32("nan")))


# ------------------------------------------------------------------------------------------------ helpers
def _isolation_model(H, bidirectional, bias, tile):
    import uvad_amd
    dev = torch.device("cuda:0")
    m = uvad_amd.PyanNet2(lstm={"hidden_size": H, "num_layers": 1, "bidirectional": bidirectional}, linear={"num_layers": 0},
                          encoding_dim=4)
    m.build()
    m.load_state_dict(cr.isolation_state_dict(H, bidirectional, bias))
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    rt.set_recurrent_tile(tile)
    rt.set_time_chunks(1)
    return m, rt


def _run(rt, x, lengths=None, lin=False):
    """-> (logits, probs, lstm tap[, feed-forward tap]) as numpy arrays."""
    lg, pr = rt.classify(x, lengths=lengths)
    y, z = rt.taps(lin=lin)
    torch.cuda.synchronize()
    out = [lg.cpu().numpy(), pr.cpu().numpy(), y.cpu().numpy()]
    if lin:
        out.append(z.cpu().numpy())
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _valid(lens, T):
    return np.arange(T)[None, :] < np.asarray(lens)[:, None]


def _worst_ratio(h, ref, bound, valid=None):
    """max |h - ref| / bound over the (valid) frames; every compared h must be finite."""
    if valid is None:
        valid = np.ones(h.shape[:2], bool)
    assert np.isfinite(h[valid]).all(), "non-finite h"
    return float((np.abs(h[valid].astype(np.float64) - ref[valid]) / bound[valid]).max())


# ------------------------------------------------------------------------------------------------ 1. cell isolation
@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_every_recurrence_form_meets_the_derived_cell_bound_on_the_edge_grid(form):
    H, bidir, tile = FORMS[form]
    D = 2 if bidir else 1
    bias = cr.isolation_biases(H, D, seed=31)
    m, rt = _isolation_model(H, bidir, bias, tile)
    x = cr.grid_values((B1, T1, 4), seed=77)
    for a, b in TWINS:
        x[a] = x[b]
    pre = cr.isolation_pre(x, bias)
    ref, bound = cr.lstm_reference(pre)
    ref_l, bound_l = cr.lstm_reference(pre, LENS1)
    valid = _valid(LENS1, T1)
    xd = torch.from_numpy(x).cuda()
    dense, ragged = {}, {}
    for mode in ("f32", "f16p", "f16p_stream"):
        rt.set_gemm_mode(mode)
        if mode != "f16p_stream":
            dense[mode] = _run(rt, xd)
            assert rt.recurrent_tile() == tile
            r = _worst_ratio(dense[mode][2], ref, bound)
            print(f"{form} dense {mode}: worst err / bound {r:.3f}")
            assert r <= 1.0, (form, mode, r)
        ragged[mode] = _run(rt, xd, lengths=LENS1)
        assert rt.recurrent_tile() == tile
        r = _worst_ratio(ragged[mode][2], ref_l, bound_l, valid)
        print(f"{form} lens  {mode}: worst err / bound {r:.3f}")
        assert r <= 1.0, (form, mode, r)
        assert not _bits(ragged[mode][0])[~valid].any() and not _bits(ragged[mode][1])[~valid].any()      # outputs past a length are exactly +0
    # the gates are exact in both GEMM modes: the same bits
    assert np.array_equal(_bits(dense["f32"][2]), _bits(dense["f16p"][2]))
    assert np.array_equal(_bits(ragged["f32"][2])[valid], _bits(ragged["f16p"][2])[valid])
    # identical pre-activations give identical bits: twin rows in other tiles, twin units in other lanes and waves
    hb = _bits(dense["f32"][2])
    for a, b in TWINS:
        assert np.array_equal(hb[a], hb[b]), (a, b)
    twins = 0
    for d in range(D):
        for j in range(24, H):
            if np.array_equal(bias[d, :, j], bias[d, :, j - 24]):
                assert np.array_equal(hb[..., d * H + j], hb[..., d * H + j - 24]), (d, j)
                twins += 1
    assert twins >= (H - 24) * D - 16 and twins > 0          # each of the 8 units with a 1e30 bias breaks at most two pairs
    # the lens run is the dense run of each row alone at T = len, bit for bit (modes f32 and f16p_stream, pinned tile)
    for mode in ("f32", "f16p_stream"):
        rt.set_gemm_mode(mode)
        for L in sorted(set(LENS1) - {0}):
            idx = [b for b, n in enumerate(LENS1) if n == L]
            lg, _, y = _run(rt, xd[idx, :L].contiguous())
            assert np.array_equal(_bits(y), _bits(ragged[mode][2][idx, :L])), (form, mode, L)
            assert np.array_equal(_bits(lg), _bits(ragged[mode][0][idx, :L])), (form, mode, L)


@gpu
@pytest.mark.parametrize("tile", [4, 16])
def test_cell_state_growing_to_300_stays_inside_the_bound(tile):
    """All four pre-activations near +40: sigma = 1, tanh(g) = 1, so c grows by 1 per step to 300 and tanh(c) saturates: exp2 of a
    very negative argument and a growing |c| (units with a -1e30 forget bias keep c small beside them)."""
    H, B, T = 128, 5, 300
    bias = cr.isolation_biases(H, 2, seed=31)
    m, rt = _isolation_model(H, True, bias, tile)
    x = np.full((B, T, 4), 40.0, np.float32)
    ref, bound = cr.lstm_reference(cr.isolation_pre(x, bias))
    assert np.abs(ref).max() <= 1.0
    hs = {}
    for mode in ("f32", "f16p"):
        rt.set_gemm_mode(mode)
        hs[mode] = _run(rt, torch.from_numpy(x).cuda())[2]
        assert rt.recurrent_tile() == tile
        r = _worst_ratio(hs[mode], ref, bound)
        print(f"tile {tile} {mode}: c up to 300, worst err / bound {r:.3f}")
        assert r <= 1.0, (tile, mode, r)
    assert np.array_equal(_bits(hs["f32"]), _bits(hs["f16p"]))


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_refined_quotients_are_correctly_rounded(form):
    """The Newton step behind v_rcp_f32 in tanh_f, quot_1 and rcp_nr makes each quotient correctly rounded (cell_ref: derivation and the
    sets such results lie in).  Observed where the cell is transparent: i / o at +40 and f at -40 give h = tanh_f(tanh_f(g)); i, f, g at
    +40 for 11 steps give tanh_f(c) = 1 and h = sigmoid(o).  A quotient without its Newton step leaves these sets on most operands."""
    H, bidir, tile = FORMS[form]
    D = 2 if bidir else 1
    T, BA, BB = 24, 16, 5
    bias = np.zeros((D, 4, H), np.float32)
    bias[:, 2] = (np.arange(H) - H // 2) / 4096.0
    bias[:, 3] = np.arange(H) / 256.0
    m, rt = _isolation_model(H, bidir, bias, tile)
    rng = np.random.default_rng(5)
    x = np.empty((BA + BB, T, 4), np.float32)
    x[:BA] = [40.0, -40.0, 0.0, 40.0]
    x[:BA, :, 2] = rng.integers(-1200, 1200, size=(BA, T)) / 4096.0
    x[BA:] = 40.0
    x[BA:, :, 3] = rng.integers(4096, 8 * 4096, size=(BB, T)) / 4096.0
    ref, bound = cr.lstm_reference(cr.isolation_pre(x, bias))
    settled = np.zeros((BB, T, D * H), bool)          # c >= 11 behind it: tanh_f(c) is exactly 1
    settled[:, 11:, :H] = True
    settled[:, :T - 11, H:] = True
    for mode in ("f32", "f16p"):
        rt.set_gemm_mode(mode)
        h = _run(rt, torch.from_numpy(x).cuda())[2]
        assert _worst_ratio(h, ref, bound) <= 1.0
        ha = np.abs(h[:BA])
        ha = ha[(ha > 2.0 ** -20) & (ha <= 1.0 / 3.0)]
        hb = h[BA:][settled]
        hb = hb[hb >= 0.71]
        ok_t, ok_s = cr.is_rounded_tanh_quotient(ha), cr.is_rounded_reciprocal(hb)
        print(f"{form} {mode}: {ok_t.mean():.4f} of {ha.size} tanh quotients, {ok_s.mean():.4f} of {hb.size} sigmoid quotients correctly rounded")
        assert ha.size > 1000 and hb.size > 1000
        assert ok_t.all() and ok_s.all(), (form, mode)


# ------------------------------------------------------------------------------------------------ 2. non-finite containment
LENS2 = [40, 12, 0, 33, 40, 7, 31, 1, 25, 40, 18, 3, 40, 22, 9, 40, 36, 2, 40, 15, 28]
# name: (hidden, layers, recurrent tile, B, T, lengths, gemm mode)
CONTAIN = {
    "h128_tile4": (128, 2, 4, 21, 40, None, "f16p"),
    "h128_tile16": (128, 2, 16, 21, 40, None, "f16p"),
    "h128_tile4_lens": (128, 2, 4, 21, 40, LENS2, "f16p"),
    "h128_tile16_lens": (128, 2, 16, 21, 40, LENS2, "f16p"),
    "h64": (64, 2, 4, 21, 40, None, "f16p"),
    "h32_generic": (32, 2, 4, 21, 40, None, "f16p"),
    "ws_projection_fused_head": (128, 4, 16, 33, 256, None, "f16p"),      # row tiles x column tiles >= 2 x CUs: the weight-stationary kernel
}


@gpu
@pytest.mark.parametrize("form", list(CONTAIN))
def test_a_non_finite_feature_stays_inside_its_sequence(form):
    """One NaN, then one +Inf, in the features of sequence 6 at frame 17 (seeded weights x2).  Every other sequence keeps the bits of the
    same call with a finite value there; the poisoned sequence is non-finite exactly where torch's CPU LSTM stack is; the next call on
    the workspace with the clean input reproduces the clean bits.
    Mode f32 compares with the clean call itself.  In mode f16p ANY feature outside the f16 range -- a finite one too -- makes the
    call's first projection run the exact kernel for every row (include/uvad.h), which moves the last bits of every sequence; the
    finite counterpart there holds 1e5 at the poisoned position, so both calls run the same kernels and the comparison isolates the
    non-finite value (the layers above and the head see it through the split kernels)."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    from oracle import torch_ref as tr
    H, L, tile, B, T, lens, split_mode = CONTAIN[form]
    F, b0, t0, f0 = 64, 6, 17, 5
    dev = torch.device("cuda:0")
    m = uvad_amd.PyanNet2(lstm={"hidden_size": H, "num_layers": L}, encoding_dim=F)
    m.build()
    seed_weights(m, 4321, 2.0)
    ref = tr.TorchPyanNet2(F, H, L, True)
    ref.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    rt.set_recurrent_tile(tile)
    x = torch.randn(B, T, F, generator=torch.Generator().manual_seed(9)) * 2.0 - 3.0
    valid = _valid(lens, T) if lens is not None else np.ones((B, T), bool)
    Lb = int(valid[b0].sum())
    assert Lb > t0
    others = np.arange(B) != b0
    names = ("logits", "probs", "lstm tap", "feed-forward tap")
    for mode in ("f32", split_mode):
        rt.set_gemm_mode(mode)
        clean = _run(rt, x.to(dev), lens, lin=True)
        assert rt.recurrent_tile() == tile
        assert all(np.isfinite(a[valid]).all() for a in clean)
        base = clean
        if mode != "f32":
            xb = x.clone()
            xb[b0, t0, f0] = 1.0e5
            base = _run(rt, xb.to(dev), lens, lin=True)
            assert all(np.isfinite(a[valid]).all() for a in base)
        for bad in (float("nan"), float("inf")):
            xp = x.clone()
            xp[b0, t0, f0] = bad
            got = _run(rt, xp.to(dev), lens, lin=True)
            v = valid[others]
            for name, a, c in zip(names, got, base):
                assert np.array_equal(_bits(a[others])[v], _bits(c[others])[v]), f"{form}, {mode}, {bad}: {name} of another sequence changed"
            want_lg, _, want_y, want_z = ref(xp[b0:b0 + 1, :Lb], taps=True)
            for name, a, w in (("logits", got[0], want_lg), ("lstm tap", got[2], want_y), ("feed-forward tap", got[3], want_z)):
                assert np.array_equal(np.isfinite(a[b0, :Lb]), np.isfinite(w[0].numpy())), \
                    f"{form}, {mode}, {bad}: {name} non-finite elsewhere than torch's"
            print(f"{form}, {mode}, {bad}: {int((~np.isfinite(got[0][b0, :Lb])).sum())} of {Lb} logits of the poisoned sequence are non-finite, "
                  f"every other sequence bit-identical")
            again = _run(rt, x.to(dev), lens, lin=True)
            for name, a, c in zip(names, again, clean):
                assert np.array_equal(_bits(a)[valid], _bits(c)[valid]), f"{form}, {mode}, {bad}: {name} of the next clean call differs"
            if lens is not None:
                assert not _bits(again[0])[~valid].any() and not _bits(got[0])[~valid].any()


# ------------------------------------------------------------------------------------------------ 3. operands at the bottom of the f16 range
@gpu
@pytest.mark.parametrize("B,T", [(5, 7), (33, 256)])      # the tile-streaming projection; large enough for the weight-stationary one
@pytest.mark.parametrize("F", [64, 80])                     # 80: padding columns up to K = 96
def test_input_projection_keeps_f16_subnormal_planes(F, B, T):
    """Features with |x| in [2^-24, 2^-14) -- their hi plane is an f16 subnormal -- under weights up to 2^10, in a matrix that also
    holds weights 2^-20 x its maximum.  Read through the transparent cell: h = tanh(tanh(z)).  A lost plane is a gross error."""
    import uvad_amd
    dev = torch.device("cuda:0")
    x, w = cr.projection_operands(F, B, T, seed=100 + F)
    z, R = cr.product_reference(x, w)
    assert np.abs(z).max() <= 0.25 and R.max() <= 4.0, (np.abs(z).max(), R.max())
    tiny = np.abs(x[..., :6].astype(np.float64)) @ np.abs(w[:, :6].astype(np.float64)).T
    assert np.median(tiny / R) > 0.02          # the f16-subnormal planes carry a real share of the sum
    ref = np.tanh(np.tanh(np.concatenate([z, z[..., ::-1]], -1)))
    Rd = np.concatenate([R, R[..., ::-1]], -1)
    m = uvad_amd.PyanNet2(lstm={"num_layers": 1}, linear={"num_layers": 0}, encoding_dim=F)
    m.build()
    m.load_state_dict(cr.projection_state_dict(w))
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    rt.set_recurrent_tile(4)
    xd = torch.from_numpy(x).to(dev)
    for mode in ("f16p", "f16p_stream", "f16p3", "f32"):
        rt.set_gemm_mode(mode)
        h = _run(rt, xd)[2]
        bound = cr.product_bound(Rd, F, mode)
        r = _worst_ratio(h, ref, bound)
        print(f"F {F}, B {B}, T {T}, {mode}: worst err / bound {r:.3f}")
        assert r <= 1.0, (F, B, T, mode, r)


@gpu
@pytest.mark.parametrize("tile", [4, 16])
def test_recurrent_product_keeps_tiny_states_and_wide_range_weights(tile):
    """W_hh (g rows only) weighs f16-subnormal h_{t-1} by up to 2^11 beside weights 2^-20 x its maximum; every step is checked from the
    TAPPED neighbour state through the transparent cell.  The 4-sequence form is an exact-f32 chain (accumulation term only); the
    16-sequence form is the split product, with P2 on the 8-bit pipe (mode f16p) and from its f16 image (f16p_stream)."""
    import uvad_amd
    dev = torch.device("cuda:0")
    B, T, H = 21, 8, 128
    s, w = cr.recurrent_operands(seed=3)
    m = uvad_amd.PyanNet2(lstm={"num_layers": 1}, linear={"num_layers": 0}, encoding_dim=4)
    m.build()
    m.load_state_dict(cr.recurrent_state_dict(s, w))
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    rt.set_recurrent_tile(tile)
    rt.set_time_chunks(1)
    x = np.zeros((B, T, 4), np.float32)
    x[..., 0] = cr.wide_range(np.random.default_rng(8), (B, T), -2, -1)
    for mode in ("f16p", "f16p_stream", "f16p3", "f32"):
        rt.set_gemm_mode(mode)
        h = _run(rt, torch.from_numpy(x).to(dev))[2]
        assert rt.recurrent_tile() == tile
        fp8 = rt.p2_on_fp8()
        assert fp8 == (mode != "f16p_stream"), (mode, fp8)      # every finite W_hh has a bf8 third plane (tests/test_host.py): no other fallback exists
        ref, R, z = cr.recurrent_reference(x[..., 0], s, w, h)
        assert np.abs(z).max() <= 0.25 and R.max() <= 4.0
        assert (np.abs(h[..., :H // 2]) < 2.0 ** -14).mean() > 0.3 and np.median(R[..., H // 2:H]) > 0.01      # tiny states, real sums
        bound = cr.product_bound(R, H, "f32" if tile == 4 else "f16p")      # the W_hh split of the 16-sequence form is exact in every mode
        r = _worst_ratio(h, ref, bound)
        print(f"tile {tile} {mode}: p2_on_fp8 {fp8}, worst err / bound {r:.3f}")
        assert r <= 1.0, (tile, mode, r)


def _head_runtime(K1, slope):
    """One-layer H = 128 model (two directions: K1 = 256, one: K1 = 128), seeded LSTM x2, wide-range head weights, the classifier's
    leaky_relu slope as given -> (runtime, head weights)."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    m = uvad_amd.PyanNet2(lstm={"num_layers": 1, "bidirectional": K1 == 256}, encoding_dim=64)
    m.build()
    seed_weights(m, 11, 2.0)
    hw = cr.head_weights(K1, seed=5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sd.update({k: torch.from_numpy(v) for k, v in hw.items()})
    rt = uvad_amd.VadRuntime(dev, model={"encoding_dim": 64, "lstm": m.hparams.lstm, "linear": m.hparams.linear, "leaky_slope": slope})
    rt.load_state_dict(sd)
    return rt, hw


def _check_head(rt, hw, K1, B, T, slope):
    x = (torch.randn(B, T, 64, generator=torch.Generator().manual_seed(4)) * 2.0 - 3.0).to(torch.device("cuda:0"))
    for mode in ("f16p_stream", "f16p", "f16p3", "f32"):
        rt.set_gemm_mode(mode)
        # the output tensors of a call are fresh allocations, which the caching allocator serves from the blocks the previous mode's
        # outputs were in: fill blocks of that size with NaN first, so that a row tile the head leaves unwritten is not finite
        # instead of holding the previous mode's (nearly equal) logits
        junk = [torch.full((B, T), float("nan"), device=x.device) for _ in range(2)]
        torch.cuda.synchronize()
        del junk
        lg, _, y = _run(rt, x)
        assert y.shape == (B, T, K1)
        ref, bound = cr.head_reference(y, hw, slope, mode)
        assert np.isfinite(lg).all() and np.abs(ref).max() > 0.05
        r = float((np.abs(lg.astype(np.float64) - ref) / bound).max())
        print(f"head K1 {K1}, B {B}, T {T}, slope {slope:g}, {mode}: worst err / bound {r:.4f} (worst |err| {float(np.abs(lg - ref).max()):.1e}, "
              f"bound there >= {float(bound.min()):.1e})")
        assert r <= 1.0, (K1, B, T, slope, mode, r)


@gpu
@pytest.mark.parametrize("B,T", [(5, 7), (33, 256)])
def test_head_on_wide_range_weights_against_a_float64_head_on_the_tapped_lstm_output(B, T):
    """linear.* and classifier weights spanning 20 octaves; the float64 head runs on the tapped LSTM output (the 22-bit planes the head
    reads in the split modes).  By the library's rule (head_fused_supported: two 128-unit layers, any row count) modes f16p / f16p3 run
    head_fused at both sizes, f16p_stream the per-layer split kernels, f32 the exact ones; the runtime has no getter for the head path,
    so the modes are what selects it here."""
    rt, hw = _head_runtime(256, 0.01)
    _check_head(rt, hw, 256, B, T, 0.01)
    rt.close()


HEAD_SLOPES = (0.01, -0.5, 0.0, 1.0, 1.5)
HEAD_T_MANY = 300


def _head_sizes(cus):
    """(B, T): one partial 64-row tile; six 64-row tiles and a partial one (12 x 37 = 444 rows); 144 tiles; and at least 1.2 x as many
    64-row tiles as CUs (65 x 300 on 256 CUs), so that workgroups of head_fused_kernel run the drawn-ahead tile loop."""
    tiles4 = -(-(12 * cus * 64) // (10 * 4 * HEAD_T_MANY))
    return {"5x7": (5, 7), "9x37": (9, 37), "33x256": (33, 256), "more_tiles_than_cus": (4 * tiles4 - 3, HEAD_T_MANY)}


@gpu
@pytest.mark.parametrize("size", ["5x7", "9x37", "33x256", "more_tiles_than_cus"])
@pytest.mark.parametrize("K1", [128, 256])
def test_fused_head_at_both_input_widths_row_counts_past_the_cu_count_and_other_slopes(K1, size):
    """The test above at K1 = 128 too (one direction: head_fused_kernel<4, 4> and <4, 3>), at row counts with a partial last 64-row tile
    and with more 64-row tiles than CUs (a workgroup then draws a second tile), and at leaky_relu slopes 0.01, -0.5, 0, 1 and 1.5 in all
    four GEMM modes.  The bound is cell_ref.head_reference's: an error entering a leaky_relu leaves it times max(1, |slope|); nothing
    is fitted.  (The static range guard of csrc/uvad_api.hip scales its activation bound by the same factor; these weights stay far
    inside the f16 range, so every split mode runs its split kernels.)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, T = _head_sizes(cus)[size]
    mt = -(-4 * ((B + 3) // 4) * T // 64)
    if size == "more_tiles_than_cus":
        assert mt >= 1.2 * cus and B % 4 == 1, (B, T, mt, cus)
    else:
        assert mt < cus, (mt, cus)
    for slope in HEAD_SLOPES:
        rt, hw = _head_runtime(K1, slope)
        _check_head(rt, hw, K1, B, T, slope)
        rt.close()
