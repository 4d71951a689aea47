"""Float64 references, derived error bounds and operand builders for tests/test_gpu_cell_edges.py and (top_of_range_operands)
tests/test_gpu_range_fallback.py (test infrastructure only).

  lstm_reference      one LSTM layer from given gate pre-activations in float64 (sigma = 1 / (1 + exp(-x)), tanh, c = f c + i g,
                      h = o tanh(c); gate order i, f, g, o; zero initial state; the backward direction runs from len - 1 down; outputs
                      at t >= len are +0), together with the elementwise bound on |h_kernel - h| that follows from the contract at
                      the top of csrc/lstm.hip: every gate function within EPS = 2^-23 (one ulp at its output scale) of the true
                      value and every f32 operation rounded once (U = 2^-24):
                          dc_t = f dc_{t-1} + |c_{t-1}| EPS + EPS dc_{t-1} + (|g| EPS + i EPS + EPS^2) + 2 U |c_t| + 2 U
                          dh_t = o (EPS + min(dc_t, 1)) + EPS + U |h_t| + EPS^2
  cell_f32 / cell1_f32  float32 restatements of lstm_cell and of the product form lstm_cell1 (csrc/lstm.hip): the same operation
                      sequence with a correctly rounded exp2 and reciprocal.  tests keep them below half the bound, which guards the
                      bound itself: hardware exp2 / reciprocal at 1 ulp each then have room.
  isolation_*         the operands that make a gate pre-activation an exactly known number through the ABI: W_hh = 0, 0/1 selection
                      rows in W_ih (encoding_dim = 4: feature g drives gate g of every unit), dyadic per-unit biases.
  transparent cell    (product_*) i / o biases +40 and f bias -40 make sigma(i) = sigma(o) = 1 in f32 and the carry < 1e-17, so the
                      LSTM tap is tanh(tanh(z)) of the matrix product z under test.
  ws_*                the library's launch-size rule for the weight-stationary projection kernel and for time chunks, restated (the
                      runtime has no getter for "which projection kernel ran": tests pick shapes the rule provably admits).
"""
import numpy as np

EPS = 2.0 ** -23          # the gate functions' contract: one ulp at their output scale
U = 2.0 ** -24            # one f32 rounding
L2E = np.float32(1.4426950408889634)

# magnitudes of the pre-activation grid: exact zeros, tiny, ordinary, around the exponent clamp (87 .. 89), far beyond it
GRID = (0.0, 2.0 ** -20, 0.25, 0.5, 1.0, 2.0, 3.5, 8.0, 17.0, 40.0, 87.0, 88.5, 89.0, 104.0, 1000.0, 3.0e4)
HUGE = 1.0e30             # a bias that puts a pre-activation outside the f16 range without touching the features


# ------------------------------------------------------------------------------------------------ float64 reference and bound
def _sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def lstm_reference(pre, lens=None, eps=EPS):
    """pre: (D, B, T, 4, H) float64 gate pre-activations (i, f, g, o) of D directions (1 = backward) -> (h, bound), both
    (B, T, D * H) float64.  lens: valid frames per row; frames past it are +0 and carry no state."""
    D, B, T, _, H = pre.shape
    lens = np.full(B, T) if lens is None else np.asarray(lens)
    h_out = np.zeros((B, T, D * H))
    b_out = np.zeros((B, T, D * H))
    u = U
    for d in range(D):
        c = np.zeros((B, H))
        dc = np.zeros((B, H))
        for s in range(T):
            t = T - 1 - s if d == 1 else s
            live = (t < lens)[:, None]
            i, f, o = _sigmoid64(pre[d, :, t, 0]), _sigmoid64(pre[d, :, t, 1]), _sigmoid64(pre[d, :, t, 3])
            g = np.tanh(pre[d, :, t, 2])
            cn = f * c + i * g
            dcn = f * dc + np.abs(c) * eps + eps * dc + (np.abs(g) * eps + i * eps + eps * eps) + 2 * u * np.abs(cn) + 2 * u
            h = o * np.tanh(cn)
            dh = o * (eps + np.minimum(dcn, 1.0)) + eps + u * np.abs(h) + eps * eps
            c = np.where(live, cn, 0.0)
            dc = np.where(live, dcn, 0.0)
            h_out[:, t, d * H:(d + 1) * H] = np.where(live, h, 0.0)
            b_out[:, t, d * H:(d + 1) * H] = np.where(live, dh, 0.0)
    return h_out, b_out


# ------------------------------------------------------------------------------------------------ float32 restatements of the kernels' cells
def _f32(x):
    return np.asarray(x, np.float32)


def _fma(a, b, c):
    """fmaf: the product of two f32 is exact in float64; the sum is rounded to float64 and then to f32 (a double rounding that differs
    from a fused operation in about one case in 2^29 and by half an ulp then)."""
    return _f32(np.float64(a) * np.float64(b) + np.float64(c))


def _exp2(a):
    with np.errstate(over="ignore", under="ignore"):
        return _f32(np.exp2(np.float64(a)))      # correctly rounded (up to the double rounding above)


def _rcp(d):
    with np.errstate(divide="ignore"):
        return _f32(1.0 / np.float64(d))


def _rcp_nr(d):
    r = _rcp(d)
    return _fma(_fma(-d, r, np.float32(1.0)), r, r)


def sigmoid_f32(x):
    x = _f32(x)
    e = _exp2(np.fmin(-L2E * x, np.float32(126.0)))      # fminf: a NaN argument gives 126
    return _rcp_nr(np.float32(1.0) + e)


def tanh_f32(x):
    x = _f32(x)
    e = _exp2((np.float32(-2.0) * L2E) * np.abs(x))
    n, d = np.float32(1.0) - e, np.float32(1.0) + e
    r = _rcp(d)
    q = n * r
    q = _fma(_fma(-d, q, n), r, q)
    return np.copysign(q, x)


def cell_f32(pre, c):
    """lstm_cell: pre (..., 4) f32 gate pre-activations, c (...) f32 -> (h, c_new) f32."""
    pre, c = _f32(pre), _f32(c)
    ig, fg, gg, og = sigmoid_f32(pre[..., 0]), sigmoid_f32(pre[..., 1]), tanh_f32(pre[..., 2]), sigmoid_f32(pre[..., 3])
    c = _fma(fg, c, ig * gg)
    return og * tanh_f32(c), c


def _quot(n, d):
    r = _rcp(d)
    q = n * r
    return _fma(_fma(-d, q, n), r, q)


def cell1_f32(pre, c):
    """lstm_cell1 (the product form of the 16-sequence kernel): one quotient per product of two gate functions."""
    pre, c = _f32(pre), _f32(c)
    one, clamp = np.float32(1.0), np.float32(125.0)
    ai, af, ao = np.fmin(pre[..., 0] * -L2E, clamp), np.fmin(pre[..., 1] * -L2E, clamp), np.fmin(pre[..., 3] * -L2E, clamp)
    ag = (np.float32(-2.0) * L2E) * np.abs(pre[..., 2])
    ei, ef, eg, eo = _exp2(ai), _exp2(af), _exp2(ag), _exp2(ao)
    itg = np.copysign(_quot(one - eg, (one + ei) * (one + eg)), pre[..., 2])
    fg = _quot(one, one + ef)
    c = _fma(fg, c, itg)
    ec = _exp2((np.float32(-2.0) * L2E) * np.abs(c))
    h = np.copysign(_quot(one - ec, (one + eo) * (one + ec)), c)
    return h, c


def run_cell_f32(cell, pre):
    """pre (N, T, 4) f32 -> h (N, T) f32 of `cell` stepped forward from zero state."""
    pre = _f32(pre)
    c = np.zeros(pre.shape[0], np.float32)
    hs = []
    for t in range(pre.shape[1]):
        h, c = cell(pre[:, t], c)
        hs.append(h)
    return np.stack(hs, 1)


# ------------------------------------------------------------------------------------------------ operands of the cell isolation
def grid_values(shape, seed):
    """Values of the pre-activation grid (float32, each exactly representable in 22 bits): a signed GRID magnitude per element, plus a
    multiple of 1/64 in [-1, 1) on about 70 % of the elements."""
    rng = np.random.default_rng(seed)
    x = np.copysign(rng.choice(np.asarray(GRID), size=shape), rng.choice([-1.0, 1.0], size=shape))      # +-0 included
    off = rng.integers(-64, 64, size=shape) / 64.0
    x = np.where(rng.random(shape) < 0.7, x + off, x)
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    return x32


def isolation_biases(H, D, seed, period=24):
    """(D, 4, H) float32 b_ih: dyadic offsets (multiples of 1/64 in [-1, 1)) that repeat every `period` units -- units `period` apart see
    identical pre-activations in other lanes and waves -- and a handful of units with +-1e30 in one gate."""
    rng = np.random.default_rng(seed)
    pat = rng.integers(-64, 64, size=(D, 4, period)) / 64.0
    b = np.stack([pat[..., j % period] for j in range(H)], -1)
    for k, (unit, gate, sign) in enumerate([(3, 0, 1), (7, 1, -1), (11, 2, 1), (13, 3, -1), (19, 2, -1), (21, 1, 1), (26, 0, -1), (29, 3, 1)]):
        b[k % D, gate, unit % H] = sign * HUGE
    return b.astype(np.float32)


def isolation_state_dict(H, bidirectional, bias, in_dim=4, lin_layers=0, seed=7):
    """torch state_dict of a one-layer PyanNet2 (encoding_dim = in_dim >= 4) whose unit j sees the pre-activations
    x[b, t, gate] + bias[d, gate, j] and nothing else: W_hh = 0, W_ih[gate H + j][gate] = 1, b_hh = 0."""
    import torch
    assert lin_layers == 0
    D = 2 if bidirectional else 1
    sd = {}
    for d in range(D):
        suf = "_l0" + ("_reverse" if d else "")
        w = np.zeros((4 * H, in_dim), np.float32)
        for g in range(4):
            w[g * H:(g + 1) * H, g] = 1.0
        sd["lstm.weight_ih" + suf] = torch.from_numpy(w)
        sd["lstm.weight_hh" + suf] = torch.zeros(4 * H, H)
        sd["lstm.bias_ih" + suf] = torch.from_numpy(np.ascontiguousarray(bias[d].reshape(4 * H)))
        sd["lstm.bias_hh" + suf] = torch.zeros(4 * H)
    g = torch.Generator().manual_seed(seed)
    sd["classifier.weight"] = (torch.rand(1, H * D, generator=g) * 2 - 1) / 8
    sd["classifier.bias"] = torch.zeros(1)
    return sd


def isolation_pre(x, bias):
    """x (B, T, 4) f32, bias (D, 4, H) f32 -> pre (D, B, T, 4, H) float64 (exact: the kernels' f32 sums are exact too, except beside a
    1e30 bias where both saturate)."""
    return x.astype(np.float64)[None, :, :, :, None] + bias.astype(np.float64)[:, None, None, :, :]


# ------------------------------------------------------------------------------------------------ operands of the split products
def wide_range(rng, shape, lo_exp, hi_exp):
    """Random signs, magnitudes 2^e (1 + m / 2^23): e uniform in [lo_exp, hi_exp), full 24-bit significands."""
    e = rng.integers(lo_exp, hi_exp, size=shape)
    m = 1.0 + rng.integers(0, 1 << 23, size=shape) / float(1 << 23)
    return (np.ldexp(m, e) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def transparent_biases(H):
    """(4 H,) f32 b_ih of the transparent cell: i / o +40 (sigma = 1 exactly in f32), f -40 (carry < 1e-17), g 0."""
    b = np.zeros((4, H), np.float32)
    b[0], b[1], b[3] = 40.0, -40.0, 40.0
    return b.reshape(4 * H)


def projection_operands(F, B, T, seed, n_tiny=6, H=128):
    """The input projection on operands at the bottom of the f16 range.  -> (x (B, T, F) f32, w_g (H, F) f32: the g rows of W_ih).
      columns 0 .. n_tiny - 1   features with |x| in [2^-24, 2^-14) (f16-subnormal hi planes) under weights in [2^4, 2^10)
      the other columns         features in [2^-6, 2^2) under weights in [2^-10 - s, 2^-7 - s), four columns at 2^-20 - s x the matrix
                                maximum; s = round(log2(max(F, 64) / 64)) octaves (0 up to F = 90, 1 at F = 128, 2 at F = 256) keep the
                                sum of F - n_tiny such terms where it is at F = 64
    The caller checks |z| <= 0.25 and R <= 4 on what comes out (tests/test_gpu_projection_forms.py does for every shape it uses).  The
    draws for H = 128, F < 91 are what they were before H and s existed."""
    rng = np.random.default_rng(seed)
    s = int(round(np.log2(max(F, 64) / 64.0)))
    x = wide_range(rng, (B, T, F), -6, 2)
    x[..., :n_tiny] = wide_range(rng, (B, T, n_tiny), -24, -14)
    w = wide_range(rng, (H, F), -10 - s, -7 - s)
    w[:, :n_tiny] = wide_range(rng, (H, n_tiny), 4, 10)
    w[0, 0] = np.float32(1023.5)                 # the matrix maximum: just below 2^10
    w[:, n_tiny:n_tiny + 4] = wide_range(rng, (H, 4), -10 - s, -9 - s)   # 2^-20 - s x the maximum
    return x, w


F16_MAX = np.float32(65504.0)                       # the first value the library's range flag catches (|x| < 65504 goes to the split)
BELOW_F16_MAX = np.nextafter(F16_MAX, np.float32(0))   # its neighbour below: hi plane = the f16 maximum, lo plane = -2^-8 x 2048 = -8


def top_of_range_operands(F, B, T, seed):
    """The input projection on operands at the TOP of the f16 range.  -> (x (B, T, F) f32, w_g (H = 128, F) f32: the g rows of W_ih).
      features  |x| = 2^15 (1 + m / 2^23) in [2^15, 65504), random signs, full significands (the hi plane's ulp is 32 there, so the lo
                plane holds up to 16 x 2048 = 32768); the first frames of row 0 (and of the last row) carry, with both signs, the
                neighbour below 65504, the ties 2^15 + 16 and 65488 (lo = +32768 after round-to-even) and the value just above the
                upper tie (hi = 65504, lo = -(16 - 2^-8) x 2048)
      weights   signed, 20 octaves [2^-41, 2^-21), full significands: every term is at most 2^-5
    The caller checks |z| <= 0.25 and R <= 4 on what comes out."""
    rng = np.random.default_rng(seed)
    H = 128
    m = rng.integers(0, (1 << 23) - 8192, size=(B, T, F))          # m = 2^23 - 8192 would be 65504 itself
    x = (np.ldexp(1.0 + m / float(1 << 23), 15) * rng.choice([-1.0, 1.0], size=(B, T, F))).astype(np.float32)
    edge = np.array([BELOW_F16_MAX, 2.0 ** 15 + 16.0, 65488.0, np.nextafter(np.float32(65488.0), np.float32(1e9))], np.float32)
    edge = np.concatenate([edge, -edge])
    for b in {0, B - 1}:
        for t in range(min(T, 4)):
            x[b, t, (np.arange(edge.size) * 7 + 3 * t + b) % F] = edge
    assert (np.abs(x) >= 2.0 ** 15).all() and (np.abs(x) < F16_MAX).all() and (np.abs(x) == BELOW_F16_MAX).any()
    w = wide_range(rng, (H, F), -41, -21)
    return x, w


def projection_state_dict(w_g, bidirectional=True, seed=7):
    """One-layer H = 128 PyanNet2 with the transparent cell: W_ih non-zero in the g rows only (= w_g, both directions), W_hh = 0."""
    import torch
    H, F = w_g.shape
    D = 2 if bidirectional else 1
    sd = {}
    for d in range(D):
        suf = "_l0" + ("_reverse" if d else "")
        w = np.zeros((4 * H, F), np.float32)
        w[2 * H:3 * H] = w_g if d == 0 else w_g[::-1]          # the backward direction holds the same rows in another order
        sd["lstm.weight_ih" + suf] = torch.from_numpy(w)
        sd["lstm.weight_hh" + suf] = torch.zeros(4 * H, H)
        sd["lstm.bias_ih" + suf] = torch.from_numpy(transparent_biases(H))
        sd["lstm.bias_hh" + suf] = torch.zeros(4 * H)
    g = torch.Generator().manual_seed(seed)
    sd["classifier.weight"] = (torch.rand(1, H * D, generator=g) * 2 - 1) / 8
    sd["classifier.bias"] = torch.zeros(1)
    return sd


def product_reference(x, w):
    """x (B, T, K) f32, w (N, K) f32 -> (z, R) float64 (B, T, N): the product and R = sum_k |w_k| |a_k|."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    return x64 @ w64.T, np.abs(x64) @ np.abs(w64).T


def product_bound(R, K, mode):
    """Bound on |h - tanh(tanh(z))| of the transparent cell, from R = sum |w| |a| and K accumulated terms.
      split modes  R (2^-21 + K 2^-24): the dropped-term bound 2^-22 of include/uvad.h doubled for the activation split, K f32
                   accumulations; f16p3 adds 2^-22 R for the dropped weight plane
      f32          the accumulation term only
      + 4 x 2^-23  the cell (two gate functions and two products, lstm_reference's bound at c_{t-1} = 0)"""
    return R * product_rel(K, mode) + 4 * EPS


# ------------------------------------------------------------------------------------------------ the launch-size rule, restated
# csrc/gemm_f16p_ws.hip (gemm_f16p_ws_supported) and csrc/uvad_api.hip (classify_impl): a projection of M = 4 ceil(B / 4) T rows onto
# N = 4 H D gate columns with K accumulated terms (the layer's input width in whole 32s) runs the weight-stationary kernel in modes
# f16p / f16p3 iff K is 64, 96, 128 or 256, N is 1 .. 8 whole 128-column tiles and ceil(M / 128) * (N / 128) >= 2 * CUs.
WS_K = (64, 96, 128, 256)


def ws_padded_k(width):
    return (width + 31) // 32 * 32


def ws_rows(B, T):
    return 4 * ((B + 3) // 4) * T


def ws_nt(H, D):
    assert (4 * H * D) % 128 == 0, (H, D)
    return 4 * H * D // 128


def ws_selected(rows, nt, K, cus):
    return K in WS_K and 1 <= nt <= 8 and (rows + 127) // 128 * nt >= 2 * cus


def ws_min_rows(nt, cus):
    """The smallest row count the rule admits at nt column tiles."""
    return (-(-2 * cus // nt) - 1) * 128 + 1


def ws_batch(nt, T, cus, above=1.05):
    """The smallest B = 1 (mod 4) -- a partial 4-sequence tile -- whose row count is at least `above` x the rule's threshold: 5 % above
    it plus at most one 4-sequence tile of 4 T rows, whatever the CU count."""
    tiles = int(np.ceil(above * ws_min_rows(nt, cus) / (4.0 * T)))
    return 4 * tiles - 3


def ws_chunks_used(rows, nt, n, cus):
    """uvad_set_time_chunks(n >= 2) is a ceiling: the count is lowered until floor(mt / n) * nt >= 2 * CUs (every chunk's projection is
    still a launch the weight-stationary kernel takes); 1 = unchunked."""
    mt = (rows + 127) // 128
    while n > 1 and (mt // n) * nt < 2 * cus:
        n -= 1
    return n


# ------------------------------------------------------------------------------------------------ correctly rounded quotients
# tanh_f, quot_1 and rcp_nr refine v_rcp_f32 by one Newton step.  On paper: r = (1 + rho) / d with |rho| <= 2^-23 (1 ulp), q0 = fl(n r)
# is within eta <= 2^-23 + 2^-24 of n / d, the residual fma(-d, q0, n) is exact, and q = fl(q0 + residual r) = fl((n / d)(1 + eta rho)):
# the quotient correctly rounded up to 2^-45 |q|.  So whatever exp2 returned, the result lies in a set that can be listed:
#     tanh_f / quot_1 with sigma = 1 beside it:  RN((1 - e) / fl(1 + e))  for an f32 e in [0.5, 1]  (1 - e is exact there: Sterbenz)
#     sigmoid_f / quot_1(1, .):                  RN(1 / d)                for an f32 d in [1, 2]
# Where f32 numbers lie denser than these sets (tanh values <= 1/3, sigmoid values >= 0.71) a quotient WITHOUT the Newton step -- two
# roundings and a 1-ulp reciprocal -- falls between the members; no tolerance is fitted to the kernel.
def _neighbours(v, k=4):
    b = _f32(v).view(np.int32)[..., None] + np.arange(-k, k + 1, dtype=np.int32)
    return b.view(np.float32)


def _is_rounded_quotient(h, n, d):
    h64, q = np.float64(h)[..., None], np.float64(n) / np.float64(d)
    ulp = np.float64(np.spacing(_f32(h)))[..., None]
    return (np.abs(h64 - q) <= 0.5 * ulp + 2.0 ** -45 * np.abs(q)).any(-1)


def is_rounded_tanh_quotient(h):
    """h f32 in (0, 1/3] -> True where h = RN((1 - e) / fl(1 + e)) (up to 2^-45) for some f32 e in [0.5, 1]."""
    h = np.abs(_f32(h))
    e = _neighbours((1.0 - np.float64(h)) / (1.0 + np.float64(h)))
    e = np.clip(e, np.float32(0.5), np.float32(1.0))
    return _is_rounded_quotient(h, np.float32(1.0) - e, np.float32(1.0) + e)


def is_rounded_reciprocal(h):
    """h f32 in [0.5, 1] -> True where h = RN(1 / d) (up to 2^-45) for some f32 d in [1, 2]."""
    h = _f32(h)
    d = np.clip(_neighbours(1.0 / np.float64(h)), np.float32(1.0), np.float32(2.0))
    return _is_rounded_quotient(h, np.float32(1.0), d)


# ------------------------------------------------------------------------------------------------ recurrent product and head (3b, 3c)
def product_rel(K, mode):
    """Relative bound (x R = sum |w| |a|) of one K-term product: see product_bound."""
    acc = K * 2.0 ** -24
    return {"f32": acc, "f16p": 2.0 ** -21 + acc, "f16p_stream": 2.0 ** -21 + acc, "f16p3": 2.0 ** -21 + 2.0 ** -22 + acc}[mode]


def recurrent_operands(seed, H=128):
    """-> (s (H,) f32, whh_g (H, H) f32).  Source units k < H / 2 take no recurrent input: their input weight s_k = 2^-2 .. 2^-24 (on
    feature 0, |x| in [0.25, 0.5)) makes h_k ordinary or tiny (below 2^-14: f16-subnormal hi planes, below 2^-24: only the lo plane
    holds it).  Target units j >= H / 2 weigh h_k by up to 2^11, so that each term is at most 2^-8 |x|, and the other targets' ordinary
    h by 2^-20 x the matrix maximum."""
    rng = np.random.default_rng(seed)
    S = H // 2
    ek = -2 - 2 * (np.arange(S) % 12)
    s = np.full(H, 2.0 ** -4, np.float32)
    s[:S] = np.ldexp(1.0, ek)
    w = np.zeros((H, H), np.float32)
    w[S:, :S] = wide_range(rng, (H - S, S), 0, 1) * np.ldexp(1.0, np.minimum(10, -ek - 9))[None, :].astype(np.float32)
    w[S:, S:] = wide_range(rng, (H - S, H - S), -10, -9)           # 2^-20 x the maximum
    w[S, 11] = np.float32(2047.0)                                   # the matrix maximum, just below 2^11
    return s, w


def recurrent_state_dict(s, whh_g, seed=7):
    """Bidirectional one-layer H = 128 model, encoding_dim = 4, transparent cell: z_t = s x_t[0] + W_hh,g h_{t-1}."""
    import torch
    H = s.shape[0]
    sd = {}
    for d in range(2):
        suf = "_l0" + ("_reverse" if d else "")
        wi = np.zeros((4 * H, 4), np.float32)
        wi[2 * H:3 * H, 0] = s
        wh = np.zeros((4 * H, H), np.float32)
        wh[2 * H:3 * H] = whh_g
        sd["lstm.weight_ih" + suf] = torch.from_numpy(wi)
        sd["lstm.weight_hh" + suf] = torch.from_numpy(wh)
        sd["lstm.bias_ih" + suf] = torch.from_numpy(transparent_biases(H))
        sd["lstm.bias_hh" + suf] = torch.zeros(4 * H)
    g = torch.Generator().manual_seed(seed)
    sd["classifier.weight"] = (torch.rand(1, 2 * H, generator=g) * 2 - 1) / 8
    sd["classifier.bias"] = torch.zeros(1)
    return sd


def recurrent_reference(x0, s, whh_g, h_tap):
    """Each step from the TAPPED neighbour state, so steps are isolated.  x0 (B, T) f32, h_tap (B, T, 2 H) f32 -> (h_ref, R, z), each
    (B, T, 2 H) float64: h_ref = tanh(tanh(z)), R = sum_k |w_k| |h_k| of the recurrent product."""
    B, T = x0.shape
    H = s.shape[0]
    h = h_tap.astype(np.float64)
    prev = np.zeros((B, T, 2 * H))
    prev[:, 1:, :H] = h[:, :-1, :H]
    prev[:, :-1, H:] = h[:, 1:, H:]
    z, R = np.zeros((B, T, 2 * H)), np.zeros((B, T, 2 * H))
    for d, w in enumerate((whh_g.astype(np.float64), whh_g.astype(np.float64))):
        sl = slice(d * H, (d + 1) * H)
        z[..., sl] = x0.astype(np.float64)[..., None] * s.astype(np.float64) + prev[..., sl] @ w.T
        R[..., sl] = np.abs(prev[..., sl]) @ np.abs(w).T
    return np.tanh(np.tanh(z)), R, z


def head_weights(K1, seed, H=128):
    """Wide-range (20 octaves, full significands) linear.0 / linear.1 / classifier weights and small biases."""
    rng = np.random.default_rng(seed)
    return {"linear.0.weight": wide_range(rng, (H, K1), -22, -2), "linear.0.bias": wide_range(rng, (H,), -12, -4),
            "linear.1.weight": wide_range(rng, (H, H), -22, -2), "linear.1.bias": wide_range(rng, (H,), -12, -4),
            "classifier.weight": wide_range(rng, (1, H), -22, -2), "classifier.bias": wide_range(rng, (1,), -6, -4)}


def head_reference(y, w, slope, mode):
    """The head in float64 on the tapped LSTM output y (B, T, K1) -> (logits, bound) (B, T).  Every layer's own error is
    R_layer x product_rel(K, mode), R_layer = sum |w| |a| + |b|.  leaky_relu is piecewise linear and continuous with slopes 1 and
    `slope`, so an error that enters it leaves it multiplied by at most max(1, |slope|) (exactly 1.0 for |slope| <= 1: the bound is then
    numerically what it was without the factor), and the next layer weighs it by |W|."""
    a, e = y.astype(np.float64), 0.0
    lip = max(1.0, abs(float(slope)))
    for wk, bk in (("linear.0.weight", "linear.0.bias"), ("linear.1.weight", "linear.1.bias"), ("classifier.weight", "classifier.bias")):
        W, b = w[wk].astype(np.float64), w[bk].astype(np.float64)
        z = a @ W.T + b
        R = np.abs(a) @ np.abs(W).T + np.abs(b)
        e = (e @ np.abs(W).T if np.ndim(e) else 0.0) + R * product_rel(W.shape[1], mode)
        if wk.startswith("classifier"):
            a = z
        else:
            a, e = np.where(z >= 0, z, slope * z), e * lip
    return a[..., 0], e[..., 0]
