"""LSTM training on the device (uvad_lstm_train_*, include/uvad.h) against tests/lstm_train_ref.py and torch on the CPU.

  exact structure   bits, no tolerance: +0 past the lengths with NaN there in x_in and dy, weight_hh gradients +0 when no row has a second
                    step, bias_ih and bias_hh bit-equal, dy = 0 and one-direction dy, a row inside a ragged batch against the row alone,
                    rows of length 0 appended, fl(gA + gB) accumulation, two runs, a captured graph of the whole step, canaries, a
                    backward call on a workspace whose header does not match
  accuracy          d_y, every parameter gradient and d_grad_in: error against float64 over the float64 tensor's max-abs, rms and max, at most
                    4 x what torch autograd in f32 on the CPU achieves on the same inputs, pooled over three seeds
  optimiser         uvad_lstm_train_apply equals the numpy-f32 Adam restatement bit for bit; twenty steps of the full chain track the
                    float64 torch loop within 4 x the deviation of torch's own f32 loop
  commit / host     uvad_classify serves the committed layers; other contexts and the frozen layers untouched; VadModel.adapt_step,
                    lstm_train_input, adapt_vad with adapt_lstm_layers = 1
"""
import ctypes as C

import numpy as np
import pytest
import torch

import head_train_ref as HR
import lstm_train_ref as R

gpu = pytest.mark.gpu
PAD = 256
CANARY = 0xA5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _dev():
    return torch.device("cuda:0")


def _runtime(Din, H, dirs, L, params=None, seed=3, scale=1.0, lin=(32, 1)):
    """A PyanNet2 of L LSTM layers (hidden H, dirs directions) on Din features with the head lin -> (runtime, state dict, model dict)."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet2(lstm={"hidden_size": H, "num_layers": L, "bidirectional": dirs == 2},
                          linear={"hidden_size": lin[0], "num_layers": lin[1]}, encoding_dim=Din)
    m.build()
    seed_weights(m, seed, scale)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    if params is not None:
        sd.update({k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in params.items()})
    md = {"encoding_dim": Din, "lstm": m.hparams.lstm, "linear": m.hparams.linear, "leaky_slope": 0.01}
    rt = uvad_amd.VadRuntime(_dev(), model=md)
    rt.load_state_dict(sd)
    return rt, sd, md


class Trainer:
    """The C entry points on buffers with canaries on both sides (the runtime's wrappers own plain buffers)."""

    def __init__(self, rt, first_layer=0, segment=32, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        from uvad_amd import _lib
        self.rt, self.lib, self.L = rt, rt.lib, _lib
        self.cfg = _lib.LstmTrainCfg(lr, betas[0], betas[1], eps, segment, first_layer)
        self.configure()
        m = rt._mc_c
        self.D = m.hidden * (2 if m.bidirectional else 1)
        self.Din = m.in_dim if first_layer == 0 else self.D
        self.P = int(self.lib.uvad_lstm_train_param_count(rt.ctx))
        self.nstate = int(self.lib.uvad_lstm_train_state_bytes(rt.ctx))
        self.sbuf = torch.full((self.nstate + 2 * PAD,), CANARY, dtype=torch.uint8, device=_dev())
        self.state = self.sbuf.data_ptr() + PAD
        self.out = torch.zeros(max(self.P, 8), dtype=torch.float32, device=_dev())
        self.ws, self.bufs = {}, []
        self.reset()

    def configure(self):
        self.rt._check(self.lib.uvad_lstm_train_configure(self.rt.ctx, C.byref(self.cfg)))

    def reset(self):
        self.configure()
        self.rt._check(self.lib.uvad_lstm_train_reset(self.rt.ctx, self.state, self.nstate, None))

    def _ws(self, B, T, key=None):
        need = int(self.lib.uvad_lstm_train_ws_bytes(self.rt.ctx, B, T))
        key = key or (B, T)
        if key not in self.ws:
            self.ws[key] = torch.full((need + 2 * PAD,), CANARY, dtype=torch.uint8, device=_dev())
        assert self.ws[key].numel() - 2 * PAD >= need
        return self.ws[key], need

    def _guarded(self, n):
        b = torch.full((n + 2 * PAD,), -7.0, dtype=torch.float32, device=_dev())
        self.bufs.append((b, n))
        return b

    def forward(self, x, lens=None, ws_key=None):
        self.configure()
        B, T = x.shape[:2]
        w, need = self._ws(B, T, ws_key)
        yb = self._guarded(B * T * self.D)
        self.rt._check(self.lib.uvad_lstm_train_forward(self.rt.ctx, x.data_ptr(), B, T, lens.data_ptr() if lens is not None else None,
                                                        yb.data_ptr() + 4 * PAD, self.state, self.nstate, w.data_ptr() + PAD, need, None))
        return yb[PAD:PAD + B * T * self.D].view(B, T, self.D)

    def backward(self, x, dy, lens=None, grad_in=True, ws_key=None):
        self.configure()
        B, T = x.shape[:2]
        w, need = self._ws(B, T, ws_key)
        gb = self._guarded(B * T * self.Din) if grad_in else None
        self.rt._check(self.lib.uvad_lstm_train_backward(self.rt.ctx, x.data_ptr(), dy.data_ptr(), B, T, lens.data_ptr() if lens is not None else None,
                                                         gb.data_ptr() + 4 * PAD if grad_in else None, self.state, self.nstate,
                                                         w.data_ptr() + PAD, need, None))
        return gb[PAD:PAD + B * T * self.Din].view(B, T, self.Din) if grad_in else None

    def apply(self):
        self.configure()
        self.rt._check(self.lib.uvad_lstm_train_apply(self.rt.ctx, self.state, self.nstate, None))

    def read(self, which):
        self.configure()
        self.rt._check(self.lib.uvad_lstm_train_read(self.rt.ctx, self.state, self.nstate, which, self.out.data_ptr(), None))
        a = self.out.cpu().numpy().copy()
        if which != self.L.HEAD_TRAIN_SCALARS:
            return a[:self.P]
        w = a[:8]
        return {"frames": int(w[2:4].view(np.uint64)[0]), "t": int(w[4:6].view(np.uint64)[0]), "bc1": w[6], "bc2": w[7]}

    def grad(self):
        return self.read(self.L.HEAD_TRAIN_GRAD)

    def canaries_intact(self):
        ok = all(bool((b[:PAD] == CANARY).all()) and bool((b[PAD + n:] == CANARY).all())
                 for b, n in [(self.sbuf, self.nstate)] + [(w, w.numel() - 2 * PAD) for w in self.ws.values()])
        return ok and all(bool((b[:PAD] == -7.0).all()) and bool((b[PAD + n:] == -7.0).all()) for b, n in self.bufs)


def _length_sets(B, T, rng):
    """The head test's five: none, every row full, every row empty, a ragged set with an empty row, a one-frame row and values that need the
    clamp, one frame each."""
    ragged = [int(v) for v in rng.integers(1, T + 1, B)]
    ragged[0] = T + 5
    if B > 1:
        ragged[1] = -3
    if B > 2:
        ragged[2] = 1
    if B == 1:
        ragged[0] = (T + 1) // 2
    return [None, [T] * B, [0] * B, ragged, [1] * B]


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _lens_d(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=_dev())


def _poisoned(x, dy, valid):
    xn, dn = x.copy(), dy.copy()
    xn[~valid], dn[~valid] = np.nan, np.nan
    return _to(xn), _to(dn)


# (Din, H, dirs, B, T): every hidden size, direction count, Din (60 is no multiple of the GEMM's k chunk), B around the 4-sequence tile and T
# around the prefetch depth; segment 32, so that with B T = 185 the segment boundaries fall inside rows (the default segment, with several
# k-chunks per segment and a ragged last one, T 500 and four layers: tests/test_gpu_train_reference_size.py)
CONFIGS = [(4, 64, 1, 1, 1), (60, 64, 2, 4, 2), (80, 128, 1, 9, 5), (256, 128, 2, 5, 37), (80, 64, 2, 5, 37)]
_SHARED = {}


def _problem(cfg):
    """Runtime, parameters and inputs of one configuration: built once, shared by the tests and left unchanged."""
    if cfg not in _SHARED:
        Din, H, dirs, B, T = cfg
        params, x, dy = R.seeded(sum(cfg), Din, H, dirs, 1, 0, B, T, scale=2.0)
        rt, _, _ = _runtime(Din, H, dirs, 1, params)
        _SHARED[cfg] = dict(rt=rt, params=params, x=x, dy=dy, shape=(Din, H, dirs, 1, 0))
    return _SHARED[cfg]


# ------------------------------------------------------------------------------------------------ exact structure
@gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_masks_zero_structure_determinism_and_closeness_over_every_length_set(cfg):
    Din, H, dirs, B, T = cfg
    p = _problem(cfg)
    rng = np.random.default_rng(7 + sum(cfg))
    tr = Trainer(p["rt"])
    assert np.array_equal(_bits(tr.read(tr.L.HEAD_TRAIN_MASTERS)), _bits(R.pack(p["params"], *p["shape"])))   # reset: the tensors as loaded
    for li, lens in enumerate(_length_sets(B, T, rng)):
        ref = R.forward_backward(p["params"], p["x"], p["dy"], H, dirs, 1, 0, lens)
        valid = ref["valid"]
        xd, dd = _poisoned(p["x"], p["dy"], valid)                                # NaN past the lengths reaches nothing
        runs = []
        for _ in range(2):
            tr.reset()
            y = tr.forward(xd, _lens_d(lens))
            gin = tr.backward(xd, dd, _lens_d(lens))
            torch.cuda.synchronize()
            runs.append((y.cpu().numpy(), gin.cpu().numpy(), tr.grad(), bytes(tr.sbuf.cpu().numpy())))
        (y, gin, g, sa), (y2, gin2, g2, sb) = runs
        assert y.tobytes() == y2.tobytes() and gin.tobytes() == gin2.tobytes() and sa == sb      # two runs: the same bytes
        assert not _bits(y[~valid]).any() and not _bits(gin[~valid]).any()        # +0 past the lengths
        assert np.isfinite(y).all() and np.isfinite(gin).all() and np.isfinite(g).all()
        assert tr.read(tr.L.HEAD_TRAIN_SCALARS)["frames"] == int(valid.sum())
        got = R.unpack(g, *p["shape"])
        n = R.lengths(B, T, lens)
        for k in got:
            if "bias_hh" in k:
                assert np.array_equal(_bits(got[k]), _bits(got[k.replace("bias_hh", "bias_ih")])), k
            if "weight_hh" in k and n.max() <= 1:
                assert not _bits(got[k]).any(), (k, li)                           # h_prev is +0 at every row's first step
            if n.max() == 0:
                assert not _bits(got[k]).any(), (k, li)
        # a sanity net under the accuracy tier (which holds the real bound): chains of at most Din + H + B T terms of f32 roundings
        for name, a, b in [("y", y, ref["y"]), ("grad_in", gin, ref["grad_in"])] + [(k, got[k], ref["grads"][k]) for k in got]:
            scale = np.abs(b).max()
            assert scale == 0.0 and not a.any() or np.abs(a - b).max() <= 1e-4 * scale, (name, li)
    assert tr.canaries_intact()


@gpu
def test_zero_dy_one_direction_dy_and_accumulation_of_two_calls():
    cfg = (80, 64, 2, 5, 37)
    Din, H, dirs, B, T = cfg
    p = _problem(cfg)
    lens = [37, 0, 1, 20, 40]
    ld = _lens_d(lens)
    valid = HR.valid_mask(B, T, lens)
    rng = np.random.default_rng(11)
    xa, da = _poisoned(p["x"], p["dy"], valid)
    xb, db = _poisoned(rng.standard_normal(p["x"].shape).astype(np.float32), rng.standard_normal(p["dy"].shape).astype(np.float32), valid)
    tr = Trainer(p["rt"])

    def one(x, d, reset=True):
        if reset:
            tr.reset()
        tr.forward(x, ld)
        tr.backward(x, d, ld, grad_in=False)
        return tr.grad()
    gA, gB = one(xa, da), one(xb, db)
    gAB = one(xa, da)
    gAB = one(xb, db, reset=False)
    assert np.array_equal(_bits(gAB), _bits(gA + gB)) and np.abs(gA).max() > 0    # the accumulator is fl(gA + gB)
    assert tr.read(tr.L.HEAD_TRAIN_SCALARS)["frames"] == 2 * int(valid.sum())
    gZ = one(xb, torch.zeros_like(db), reset=False)                               # dy = 0: no accumulator bit changes
    assert np.array_equal(_bits(gZ), _bits(gAB))
    for d in range(2):                                                            # dy in one direction's half only: the other direction's tensors stay +0
        half = p["dy"].copy()
        half[..., (1 - d) * H:(2 - d) * H] = 0.0
        g = R.unpack(one(xa, _to(half)), *p["shape"])
        for k, v in g.items():
            other = k.endswith("_reverse") == (d == 0)
            assert bool(_bits(v).any()) != other, (d, k)
    assert tr.canaries_intact()


@gpu
@pytest.mark.parametrize("cfg", [(60, 64, 2, 4, 2), (256, 128, 2, 5, 37), (80, 128, 1, 9, 5)])
def test_a_row_inside_a_ragged_batch_equals_the_row_alone_and_empty_rows_change_nothing(cfg):
    Din, H, dirs, B, T = cfg
    p = _problem(cfg)
    rng = np.random.default_rng(5)
    lens = _length_sets(B, T, rng)[3]
    n = R.lengths(B, T, lens)
    valid = HR.valid_mask(B, T, lens)
    xd, dd = _poisoned(p["x"], p["dy"], valid)
    tr = Trainer(p["rt"])
    y = tr.forward(xd, _lens_d(lens))
    gin = tr.backward(xd, dd, _lens_d(lens))
    g = tr.grad()
    for b in range(B):
        if n[b] == 0:
            continue
        one = Trainer(p["rt"])
        x1, d1 = xd[b:b + 1, :n[b]].contiguous(), dd[b:b + 1, :n[b]].contiguous()
        y1 = one.forward(x1)
        g1 = one.backward(x1, d1)
        assert torch.equal(y1[0], y[b, :n[b]]) and torch.equal(g1[0], gin[b, :n[b]]), b
        assert one.canaries_intact()
    # three rows of length 0 appended (their frames hold NaN): no gradient bit changes
    more = Trainer(p["rt"])
    xe = torch.cat([xd, torch.full((3, T, Din), float("nan"), device=_dev())])
    de = torch.cat([dd, torch.full((3, T, H * dirs), float("nan"), device=_dev())])
    le = _lens_d(list(lens) + [0, -1, 0])
    ye = more.forward(xe, le)
    ge = more.backward(xe, de, le)
    assert np.array_equal(_bits(more.grad()), _bits(g))
    assert torch.equal(ye[:B], y) and torch.equal(ge[:B], gin) and not ye[B:].any() and not ge[B:].any()
    assert tr.canaries_intact() and more.canaries_intact()


@gpu
def test_backward_on_a_workspace_of_another_shape_writes_nothing():
    cfg = (60, 64, 2, 4, 2)
    Din, H, dirs, B, T = cfg
    p = _problem(cfg)
    tr = Trainer(p["rt"])
    x, dy = _to(p["x"]), _to(p["dy"])
    tr.forward(x, ws_key="w")
    tr.backward(x, dy, grad_in=False, ws_key="w")
    torch.cuda.synchronize()
    before, ws_before = bytes(tr.sbuf.cpu().numpy()), bytes(tr.ws["w"].cpu().numpy())
    xs, ds = x.reshape(T, B, Din), dy.reshape(T, B, H * dirs)                      # B and T swapped: the same workspace size, another header
    gin = tr.backward(xs, ds, ws_key="w")
    torch.cuda.synchronize()
    assert bytes(tr.sbuf.cpu().numpy()) == before and bytes(tr.ws["w"].cpu().numpy()) == ws_before
    assert bool((gin == -7.0).all())                                               # d_grad_in was not written either
    tr.ws["w"][PAD:PAD + 4] = 0                                                    # ... and a workspace without the magic word
    gin = tr.backward(x, dy, ws_key="w")
    torch.cuda.synchronize()
    assert bytes(tr.sbuf.cpu().numpy()) == before and bool((gin == -7.0).all())
    assert tr.canaries_intact()


# ------------------------------------------------------------------------------------------------ accuracy
def _pooled_ratios(cases, layers, first, refs=None):
    """cases: [(params, x, dy, lens, kernel outputs {name: array})] -> {name: (kernel rms, kernel max, torch rms, torch max)} pooled.
    refs: per case the (float64 restatement, torch f32) pair where the caller shares them; None: computed here."""
    pool = {}
    for ci, (params, x, dy, lens, got, shape) in enumerate(cases):
        Din, H, dirs = shape[:3]
        if refs is not None:
            truth, cpu = refs[ci]
        else:
            truth = R.forward_backward(params, x, dy, H, dirs, layers, first, lens)
            cpu = R.torch_forward_backward(params, x, dy, H, dirs, layers, first, lens, dtype=torch.float32)
        names = [("y", truth["y"], cpu["y"]), ("grad_in", truth["grad_in"], cpu["grad_in"])]
        names += [(k, truth["grads"][k], cpu["grads"][k]) for k in truth["grads"]]
        for k, t, c in names:
            scale = np.abs(t).max()
            for who, a in (("kernel", got[k]), ("torch", c)):
                e = np.abs(np.asarray(a, np.float64).reshape(t.shape) - t) / scale
                pool.setdefault((k, who), []).append((float(np.sqrt((e ** 2).mean())), float(e.max())))
    out = {}
    for (k, who), v in pool.items():
        a = np.array(v)
        out.setdefault(k, {})[who] = (float(np.sqrt((a[:, 0] ** 2).mean())), float(a[:, 1].max()))
    return out


def _accuracy(Din, H, dirs, layers, B, T, lens):
    cases = []
    for seed in range(3):
        shape = (Din, H, dirs, layers, 0)
        params, x, dy = R.seeded(100 + seed, *shape, B, T, scale=2.0)
        rt, _, _ = _runtime(Din, H, dirs, layers, params)
        tr = Trainer(rt, segment=32)
        valid = HR.valid_mask(B, T, lens)
        xd, dd = _poisoned(x, dy, valid)
        y = tr.forward(xd, _lens_d(lens))
        gin = tr.backward(xd, dd, _lens_d(lens))
        got = dict(R.unpack(tr.grad(), *shape), y=y.cpu().numpy(), grad_in=gin.cpu().numpy())
        assert tr.canaries_intact()
        cases.append((params, x, dy, lens, got, shape))
        rt.close()
    worst = 0.0
    for k, f in _pooled_ratios(cases, layers, 0).items():
        ratios = (f["kernel"][0] / f["torch"][0], f["kernel"][1] / f["torch"][1])
        worst = max(worst, *ratios)
        print(f"{k}: kernel rms {f['kernel'][0]:.2e} max {f['kernel'][1]:.2e} | torch f32 rms {f['torch'][0]:.2e} max {f['torch'][1]:.2e} | "
              f"ratios {ratios[0]:.2f} {ratios[1]:.2f}")
    return worst


@gpu
@pytest.mark.parametrize("Din,H,dirs,layers,B,T,lens", [(256, 128, 2, 1, 5, 37, [37, 30, 12, 37, 5]), (80, 64, 2, 1, 3, 19, [19, 7, 19]),
                                                        (80, 64, 2, 2, 3, 19, [19, 7, 19])])
def test_output_and_gradients_within_four_times_torch_f32_autograd(Din, H, dirs, layers, B, T, lens):
    """Per tensor, rms and max error against the float64 restatement divided by that tensor's float64 max-abs, pooled over three seeds (rms:
    root of the mean square over the seeds; max: the largest), for the kernels and for torch.nn.LSTM autograd in f32 on the CPU on the same
    inputs; the kernels may be at most 4 x torch (DESIGN.md 3.25's bound for k-ordered chains against torch's blocked sums).  layers = 2
    covers the hand-off of d_in to the next lower layer's dy."""
    assert _accuracy(Din, H, dirs, layers, B, T, lens) <= 4.0


# ------------------------------------------------------------------------------------------------ optimiser and training
@gpu
def test_apply_equals_the_f32_adam_restatement_bit_for_bit():
    cfg = (80, 64, 2, 5, 37)
    p = _problem(cfg)
    hyper = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
    tr = Trainer(p["rt"], **hyper)
    lens = [37, 0, 1, 20, 40]
    valid = HR.valid_mask(5, 37, lens)
    xd, dd = _poisoned(p["x"], p["dy"], valid)
    ld, zero = _lens_d(lens), _lens_d([0] * 5)
    w, st = tr.read(tr.L.HEAD_TRAIN_MASTERS), HR.adam_init(tr.P)
    for step in range(7):
        for _ in range(1 + step % 2):                                             # one and two accumulated calls
            tr.forward(xd, ld)
            tr.backward(xd, dd, ld, grad_in=False)
        acc, s = tr.grad(), tr.read(tr.L.HEAD_TRAIN_SCALARS)
        assert s["frames"] == int(valid.sum()) * (1 + step % 2) and s["t"] == step and np.abs(acc).max() > 0
        tr.apply()
        w, st = HR.adam_step(w, acc, s["frames"], st, lr=hyper["lr"], beta1=0.9, beta2=0.999, eps=1e-8)
        for which, want in ((tr.L.HEAD_TRAIN_MASTERS, w), (tr.L.HEAD_TRAIN_M, st["m"]), (tr.L.HEAD_TRAIN_V, st["v"])):
            assert np.array_equal(_bits(tr.read(which)), _bits(want)), (step, which)
        s = tr.read(tr.L.HEAD_TRAIN_SCALARS)
        assert s["t"] == step + 1 and s["frames"] == 0 and not tr.grad().any()
        assert _bits(s["bc1"]) == _bits(st["bc1"]) and _bits(s["bc2"]) == _bits(st["bc2"])
    before = bytes(tr.sbuf.cpu().numpy())
    tr.apply()                                                                    # nothing accumulated: no step
    tr.forward(xd, zero)
    tr.backward(xd, dd, zero, grad_in=False)                                      # a call without a valid frame, then a step: still none
    tr.apply()
    assert bytes(tr.sbuf.cpu().numpy()) == before and tr.canaries_intact()


def _torch_model(sd, Din, H, dtype, layers=1):
    """The seeded bidirectional model of `layers` layers with the head 32 / 1 as torch modules on the CPU -> (parameters, forward(x, lens) -> p (B, T))."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    lstm = torch.nn.LSTM(Din, H, layers, batch_first=True, bidirectional=True).to(dtype)
    with torch.no_grad():
        for name, prm in lstm.named_parameters():
            prm.copy_(sd["lstm." + name].to(dtype))
    head = {k: sd[k].detach().clone().to(dtype).requires_grad_(True) for k in ("linear.0.weight", "linear.0.bias", "classifier.weight", "classifier.bias")}

    def fwd(x, lens):
        out, _ = lstm(pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False))
        out, _ = pad_packed_sequence(out, batch_first=True, total_length=x.shape[1])
        out = torch.nn.functional.leaky_relu(torch.nn.functional.linear(out, head["linear.0.weight"], head["linear.0.bias"]), 0.01)
        return torch.sigmoid(torch.nn.functional.linear(out, head["classifier.weight"], head["classifier.bias"])).squeeze(-1)
    return list(lstm.parameters()) + list(head.values()), fwd


@gpu
def test_twenty_steps_of_the_full_chain_track_the_float64_torch_loop():
    """H 64, one bidirectional layer, head 32 / 1, B 4, T 37, ragged: the rms deviation of the 20 losses from the float64 torch loop, pooled
    over three seeds, at most 4 x the deviation of torch's own f32 loop; the loss ends below where it started."""
    Din, H, B, T, lr = 80, 64, 4, 37, 3e-3
    lens = [37, 21, 9, 30]
    valid = HR.valid_mask(B, T, lens)
    v = torch.from_numpy(valid)
    dev2 = {"kernel": [], "torch": []}
    for seed in range(3):
        rt, sd, _ = _runtime(Din, H, 2, 1, seed=40 + seed, scale=2.0)
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((B, T, Din)).astype(np.float32)
        y = (x[..., :8].sum(-1) > 0).astype(np.uint8)
        loops = {}
        for dtype in (torch.float64, torch.float32):
            prm, fwd = _torch_model(sd, Din, H, dtype)
            opt = torch.optim.Adam(prm, lr=lr)
            xt, yt, losses = torch.tensor(x, dtype=dtype), torch.from_numpy(y).to(dtype), []
            for _ in range(20):
                opt.zero_grad()
                loss = torch.nn.functional.binary_cross_entropy(fwd(xt, lens)[v], yt[v])
                losses.append(loss.item())
                loss.backward()
                opt.step()
            loops[dtype] = np.array(losses)
        hh, hl = rt.head_train_open(lr=lr), rt.lstm_train_open(layers=1, lr=lr)
        xd, yd, ld = _to(x), _to(y), _lens_d(lens)
        got = []
        for _ in range(20):
            out = rt.lstm_train_forward(hl, xd, lengths=ld)
            _, gx = rt.head_train_grad(hh, out, yd, lengths=ld, want_grad_x=True)
            rt.lstm_train_backward(hl, xd, gx, lengths=ld)
            got.append(rt.head_train_batch_loss(hh).clone())
            rt.head_train_apply(hh)
            rt.lstm_train_apply(hl)
        torch.cuda.synchronize()
        got = np.array([float(l) for l in got])
        want = loops[torch.float64]
        dev2["kernel"].append(float(((got - want) ** 2).mean()))
        dev2["torch"].append(float(((loops[torch.float32] - want) ** 2).mean()))
        print(f"seed {seed}: loss {want[0]:.6f} -> {want[19]:.6f} (float64), kernel {got[0]:.6f} -> {got[19]:.6f}")
        assert got[19] < got[0] and want[19] < want[0]
        assert rt.lstm_train_read(hl)["step"] == 20
        rt.close()
    k, t = (float(np.sqrt(np.mean(dev2[w]))) for w in ("kernel", "torch"))
    print(f"rms deviation of 20 losses from the float64 loop, three seeds: kernel {k:.3e}, torch f32 {t:.3e}, ratio {k / t:.2f}")
    assert k <= 4.0 * t


@gpu
def test_a_captured_graph_of_the_whole_step_replays_to_the_eager_bytes():
    Din, H, B, T, lr = 80, 64, 4, 37, 3e-3
    rt, _, _ = _runtime(Din, H, 2, 1, seed=9, scale=2.0)
    rng = np.random.default_rng(2)
    batches = []
    for k in range(5):
        x = rng.standard_normal((B, T, Din)).astype(np.float32)
        batches.append((_to(x), _to((x[..., :8].sum(-1) > 0).astype(np.uint8)), _lens_d([T - k, 21 + k, 9, 30])))

    def step(hh, hl, x, y, n):
        out = rt.lstm_train_forward(hl, x, lengths=n)
        _, gx = rt.head_train_grad(hh, out, y, lengths=n, want_grad_x=True)
        rt.lstm_train_backward(hl, x, gx, lengths=n)
        rt.head_train_apply(hh)
        rt.lstm_train_apply(hl)
    eh, el = rt.head_train_open(lr=lr), rt.lstm_train_open(layers=1, lr=lr)
    for x, y, n in batches:
        step(eh, el, x, y, n)
    gh, gl = rt.head_train_open(lr=lr), rt.lstm_train_open(layers=1, lr=lr)
    sx, sy, sl = torch.zeros_like(batches[0][0]), torch.zeros((B, T), dtype=torch.uint8, device=_dev()), torch.zeros(B, dtype=torch.int32, device=_dev())
    step(gh, gl, sx, sy, sl)                                                      # sizes the workspaces; no valid frame, nothing accumulated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                 # one stream; a synchronisation or allocation would fail here
        step(gh, gl, sx, sy, sl)
    assert rt.lstm_train_read(gl)["step"] == 0 and rt.head_train_read(gh)["step"] == 0   # captured, not run
    for x, y, n in batches:
        sx.copy_(x), sy.copy_(y), sl.copy_(n)
        graph.replay()
    torch.cuda.synchronize()
    assert bytes(el["state"].cpu().numpy()) == bytes(gl["state"].cpu().numpy())
    assert bytes(eh["state"].cpu().numpy()) == bytes(gh["state"].cpu().numpy())
    assert rt.lstm_train_read(gl)["step"] == 5
    rt.close()


# ------------------------------------------------------------------------------------------------ commit and host layer
@gpu
def test_commit_serves_the_adapted_layers_and_leaves_frozen_layers_and_other_contexts_alone():
    import uvad_amd
    Din, H, B, T = 64, 64, 3, 50
    rt, sd, md = _runtime(Din, H, 2, 2, seed=21, scale=2.0)
    other = uvad_amd.VadRuntime(_dev(), model=md)
    other.load_state_dict(sd)
    g = torch.Generator().manual_seed(4)
    feats = (torch.randn(B, T, Din, generator=g) * 2.0 - 1.0).to(_dev())
    y = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8).to(_dev())
    lg0 = rt.classify(feats)[0].clone()
    x_in = rt.lstm_train_input(feats, layers=1).clone()
    first = uvad_amd.VadRuntime(_dev(), model=dict(md, lstm=dict(md["lstm"], num_layers=1)))   # the sibling's tap, built by hand
    first.load_state_dict({k: v for k, v in sd.items() if "_l1" not in k})
    first.classify(feats, want_probs=False)
    assert torch.equal(x_in, first.taps(lin=False)[0])
    assert [k for k, _ in rt.lstm_train_keys(1)] == [k for k, _ in R.keys(2 * H, H, 2, 2, 1)]
    hh, hl = rt.head_train_open(lr=1e-2), rt.lstm_train_open(layers=1, lr=1e-2)
    for _ in range(3):
        out = rt.lstm_train_forward(hl, x_in)
        _, gx = rt.head_train_grad(hh, out, y, want_grad_x=True)
        rt.lstm_train_backward(hl, x_in, gx)
        rt.head_train_apply(hh)
        rt.lstm_train_apply(hl)
    rt.lstm_train_commit(hl)
    rt.head_train_commit(hh)
    lg1 = rt.classify(feats)[0].clone()
    new = dict(sd)
    lsd = rt.lstm_train_state_dict(hl)
    new.update(lsd)
    new.update(rt.head_train_state_dict(hh))
    assert list(lsd) == [k for k, _ in R.keys(2 * H, H, 2, 2, 1)] and all(not torch.equal(lsd[k], sd[k]) for k in lsd)
    fresh = uvad_amd.VadRuntime(_dev(), model=md)
    fresh.load_state_dict(new)                                                    # layer 0 as it was, layer 1 and the head as read back
    assert torch.equal(fresh.classify(feats)[0], lg1)                             # bit-identical: the frozen layer is untouched
    assert float((lg1 - lg0).abs().max()) > 1e-3
    assert torch.equal(other.classify(feats)[0], lg0)                             # another context is unaffected
    assert torch.equal(rt.lstm_train_input(feats, layers=1), x_in)
    for r in (other, first, fresh, rt):
        r.close()


@gpu
def test_vadmodel_adapt_step_and_adapt_commit_put_the_adapted_tensors_into_the_state_dict():
    from uvad_amd.engine import VadModel
    from uvad_amd.synth import seed_weights
    md = {"encoding_dim": 64, "lstm": {"hidden_size": 64, "num_layers": 2}, "linear": {"hidden_size": 32, "num_layers": 1}}
    vm = VadModel("PyanNet2", md, learning_rate=3e-3)
    seed_weights(vm.model, 77, 2.0)
    vm = vm.to(_dev()).eval()
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(2, 60, 64, generator=g) * 2.0 - 1.0).to(_dev())
    y = (torch.rand(2, 60, generator=g) < 0.5).to(torch.uint8)
    batch = {"inputs": x, "is_voice": y, "lengths": [60, 33]}
    with pytest.raises(NotImplementedError):
        vm.training_step({}, 0)
    cached = dict(batch, lstm_in=vm.lstm_in(batch, 1).clone())
    vm2 = VadModel("PyanNet2", md, learning_rate=3e-3)
    vm2.load_state_dict(vm.state_dict())
    vm2 = vm2.to(_dev()).eval()
    la = [vm.adapt_step(batch, i, accumulate=2, lstm_layers=1) for i in range(4)]
    lb = [vm2.adapt_step(cached, i, accumulate=2, lstm_layers=1) for i in range(4)]
    torch.cuda.synchronize()
    assert all(t.is_cuda and t.dim() == 0 for t in la)
    assert [float(t) for t in la] == [float(t) for t in lb]                        # the cached prefix: the same bits
    assert float(la[1]) == float(la[0]) and float(la[2]) < float(la[0])            # a step after every second call
    before = {k: v.clone() for k, v in vm.state_dict().items()}
    vm.adapt_commit()
    vm2.adapt_commit()
    after = vm.state_dict()
    for k in before:
        learns = k.startswith(("model.linear.", "model.classifier.")) or (k.startswith("model.lstm.") and "_l1" in k)
        assert (not torch.equal(before[k], after[k])) == learns, k
        assert torch.equal(after[k], vm2.state_dict()[k])
    assert vm.model._rt_stamp == vm.model._stamp(_dev())                          # the committed runtime is served as it is
    assert torch.isfinite(vm(x)).all()


@gpu
def test_a_sincnet_context_trains_its_only_lstm_layer_on_the_sincnet_output():
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet(lstm={"num_layers": 1}, linear={"hidden_size": 64, "num_layers": 1})
    m.build()
    seed_weights(m, 21, 2.0)
    m = m.to(_dev()).eval()
    rt = m.runtime(_dev())
    wav = torch.randn(2, 16000, generator=torch.Generator().manual_seed(2)).to(_dev()) * 0.1
    feats = rt.sincnet(wav)
    lg0 = rt.classify(feats)[0].clone()
    B, T = lg0.shape
    y = torch.from_numpy((np.random.default_rng(0).random((B, T)) < 0.5).astype(np.uint8)).to(_dev())
    x_in = rt.lstm_train_input(feats, layers=1)
    assert x_in.data_ptr() == feats.data_ptr()                                    # first_layer 0: the SincNet output itself
    hh, hl = rt.head_train_open(lr=1e-2), rt.lstm_train_open(layers=1, lr=1e-2)
    out = rt.lstm_train_forward(hl, x_in)
    _, gx = rt.head_train_grad(hh, out, y, want_grad_x=True)
    gin = rt.lstm_train_backward(hl, x_in, gx, want_grad_in=True)
    rt.head_train_apply(hh)
    rt.lstm_train_apply(hl)
    assert rt.lstm_train_read(hl)["step"] == 1 and tuple(gin.shape) == tuple(feats.shape) and torch.isfinite(gin).all() and bool(gin.any())
    rt.lstm_train_commit(hl)
    rt.head_train_commit(hh)
    lg1, _ = m.forward_logits(wav)
    assert torch.isfinite(lg1).all() and float((lg1 - lg0).abs().max()) > 1e-3


@gpu
def test_adapt_vad_with_one_lstm_layer_runs_an_epoch_and_writes_its_checkpoint(tmp_path):
    import wave
    import main as entry
    from config.config import load_config
    from uvad_amd.synth import synth_pcm
    paths, labels = [], []
    for k, secs in enumerate((1.5, 2.1)):
        x = synth_pcm(1, int(secs * 16000), seed=900 + k)[0]
        x[int(0.5 * 16000):int(1.0 * 16000)] *= 0.02
        p, f = tmp_path / f"a{k}.wav", tmp_path / f"a{k}.txt"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
        f.write_text(f"0.0\t0.5\tSPC\n1.0\t{secs}\tSPC\n")
        paths.append(str(p)); labels.append(str(f))
    cfg = load_config()
    assert cfg.adapt_lstm_layers == 0                                             # the default: the head alone
    cfg.model_dict.encoding_dim = 64
    cfg.model_dict.lstm = {"hidden_size": 64, "num_layers": 2}
    cfg.weights_scale = 2.0
    cfg.input.kind, cfg.input.paths, cfg.input.labels = "wav", paths, labels
    cfg.function, cfg.learning_rate, cfg.max_epochs, cfg.check_val_every_n_epoch, cfg.adapt_lstm_layers = "adapt", 3e-3, 1, 1, 1
    cfg.adapted_checkpoint_path = str(tmp_path / "out" / "adapted.ckpt")
    got = entry.main(cfg)
    assert [e for e, _ in got["val_loss"]] == [0, 1] and len(got["train_loss"]) == 1 and np.isfinite(got["train_loss"][0])
    blob = torch.load(got["checkpoint_path"], weights_only=True)
    assert blob["epoch"] == 1 and blob["global_step"] == 2 and all(k.startswith("model.") for k in blob["state_dict"])
    fresh = load_config()
    fresh.model_dict.encoding_dim, fresh.model_dict.lstm = 64, {"hidden_size": 64, "num_layers": 2}
    from uvad_amd.engine import VadModel
    from uvad_amd.synth import seed_weights
    ref = VadModel("PyanNet2", dict(fresh.model_dict))
    seed_weights(ref.model, cfg.weights_seed, 2.0)
    base = ref.state_dict()
    moved = {k for k, v in blob["state_dict"].items() if not torch.equal(v, base[k].cpu())}
    assert moved and all(k.startswith(("model.linear.", "model.classifier.")) or "_l1" in k for k in moved)
    assert any("lstm.weight_hh_l1" in k for k in moved)
