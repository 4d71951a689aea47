"""Head fine-tuning on the device (uvad_head_train_*, include/uvad.h) against tests/head_train_ref.py.

  exact tier      controlled operands (integer x0, sparse weights in {-1, 0, 1}, slope 0.5, integer dz through d_dz): every sum is exact in
                  f32 in any order (asserted on the CPU first), so the accumulated gradient of every tensor and d_grad_x equal the float64
                  restatement bit for bit over every tile count, length set, segment and number of accumulated calls; NaN past the
                  lengths, canaries around every buffer
  loss tier       dz recomputed in numpy f32 from the returned p is the gradient the kernel used (through a head without feed-forward
                  layers: d_grad_x = dz w_c), the bias gradient and the loss sum inside the summation bounds, the loss equal to uvad_score_step's
  accuracy tier   the seeded 128 / 2 head on real taps: error against float64 at most 4 x what torch.autograd in f32 on the CPU achieves
  optimiser       uvad_head_train_apply equals the numpy-f32 Adam restatement bit for bit; twenty steps track the float64 torch loop;
                  a captured graph of grad + apply replays to the eager bytes; two runs are byte-identical
  commit / host   uvad_classify serves the adapted head, the encoder tap and other contexts are unaffected; VadModel.adapt_head_*
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import head_train_ref as R

gpu = pytest.mark.gpu
PAD = 256
CANARY = 0xA5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _dev():
    return torch.device("cuda:0")


def _head_runtime(D0, H, L, slope, params=None, seed=3):
    """A one-layer bidirectional model of hidden D0 / 2 with the head (H, L) and the given head tensors -> (runtime, state dict)."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    lstm = {"hidden_size": D0 // 2, "num_layers": 1, "bidirectional": True}
    lin = {"hidden_size": H if L else 32, "num_layers": L}
    m = uvad_amd.PyanNet2(lstm=lstm, linear=lin, encoding_dim=4)
    m.build()
    seed_weights(m, seed, 1.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    if params is not None:
        sd.update({k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in params.items()})
    rt = uvad_amd.VadRuntime(_dev(), model={"encoding_dim": 4, "lstm": m.hparams.lstm, "linear": m.hparams.linear, "leaky_slope": slope})
    rt.load_state_dict(sd)
    return rt, sd


class Trainer:
    """The C entry points on buffers with canaries on both sides (the runtime's wrappers own plain buffers)."""

    def __init__(self, rt, segment=0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        from uvad_amd import _lib
        self.rt, self.lib, self.L = rt, rt.lib, _lib
        self.cfg = _lib.HeadTrainCfg(lr, betas[0], betas[1], eps, segment)
        self.configure()
        self.P = int(self.lib.uvad_head_train_param_count(rt.ctx))
        self.nstate = int(self.lib.uvad_head_train_state_bytes(rt.ctx))
        self.sbuf = torch.full((self.nstate + 2 * PAD,), CANARY, dtype=torch.uint8, device=_dev())
        self.state = self.sbuf.data_ptr() + PAD
        self.out = torch.zeros(max(self.P, 8), dtype=torch.float32, device=_dev())
        self.ws = {}
        self.reset()

    def configure(self):
        self.rt._check(self.lib.uvad_head_train_configure(self.rt.ctx, C.byref(self.cfg)))

    def reset(self):
        self.configure()
        self.rt._check(self.lib.uvad_head_train_reset(self.rt.ctx, self.state, self.nstate, None))

    def grad(self, x, lens=None, gt=None, fw=None, dz=None, probs=None, grad_x=None):
        """Tensors on the device; probs / grad_x: (tensor, pointer of its first element, ld) or None."""
        self.configure()
        B, T = x.shape[:2]
        need = int(self.lib.uvad_head_train_ws_bytes(self.rt.ctx, B, T))
        if (B, T) not in self.ws:
            self.ws[(B, T)] = torch.full((need + 2 * PAD,), CANARY, dtype=torch.uint8, device=_dev())
        w = self.ws[(B, T)]
        p = lambda t: (t.data_ptr(), t.stride(0)) if t is not None else (None, 0)
        self.rt._check(self.lib.uvad_head_train_grad(self.rt.ctx, x.data_ptr(), B, T, lens.data_ptr() if lens is not None else None, *p(gt), *p(fw),
                                                     *p(dz), *(probs[1:] if probs else (None, 0)), grad_x[1] if grad_x else None,
                                                     self.state, self.nstate, w.data_ptr() + PAD, need, None))
        return w

    def apply(self):
        self.configure()
        self.rt._check(self.lib.uvad_head_train_apply(self.rt.ctx, self.state, self.nstate, None))

    def read(self, which):
        self.configure()
        self.rt._check(self.lib.uvad_head_train_read(self.rt.ctx, self.state, self.nstate, which, self.out.data_ptr(), None))
        a = self.out.cpu().numpy().copy()
        if which != self.L.HEAD_TRAIN_SCALARS:
            return a[:self.P]
        w = a[:8]
        return {"loss": float(w[0:2].view(np.float64)[0]), "frames": int(w[2:4].view(np.uint64)[0]), "t": int(w[4:6].view(np.uint64)[0]),
                "bc1": w[6], "bc2": w[7]}

    def canaries_intact(self):
        bufs = [(self.sbuf, self.nstate)] + [(w, w.numel() - 2 * PAD) for w in self.ws.values()]
        return all(bool((b[:PAD] == CANARY).all()) and bool((b[PAD + n:] == CANARY).all()) for b, n in bufs)


def _length_sets(B, T, rng):
    """Five: none, every row full, every row empty, a ragged set with an empty and a full row whose values need the clamp, one frame each."""
    ragged = [int(v) for v in rng.integers(1, T + 1, B)]
    ragged[0] = T + 5
    if B > 1:
        ragged[1] = -3
    if B == 1:
        ragged[0] = (T + 1) // 2
    return [None, [T] * B, [0] * B, ragged, [1] * B]


SHAPES = [(1, 1), (1, 127), (3, 129), (2, 301)]
HEADS = [(D0, H, L) for D0 in (64, 128, 256) for H in (32, 128) for L in (0, 1, 2) if L or H == 32]


# ------------------------------------------------------------------------------------------------ exact tier
@gpu
@pytest.mark.parametrize("D0,H,L", HEADS)
def test_contractions_masks_tiles_and_fold_are_exact_on_controlled_operands(D0, H, L):
    from uvad_amd import _lib
    rng = np.random.default_rng(1000 + D0 + 7 * H + L)
    params = {}
    for k, shape in R.keys(D0, H, L):
        dens = min(1.0, 6.0 / shape[-1]) if len(shape) == 2 else 1.0
        params[k] = (rng.integers(-1, 2, shape) * (rng.random(shape) < dens)).astype(np.float32)
    rt, _ = _head_runtime(D0, H, L, 0.5, params)
    trainers = {seg: Trainer(rt, segment=seg) for seg in (32, 64, 0)}
    for tr in trainers.values():
        assert np.array_equal(_bits(tr.read(_lib.HEAD_TRAIN_MASTERS)), _bits(R.pack(params, D0, H, L)))   # reset: the finalized head tensors
    for B, T in SHAPES:
        for li, lens in enumerate(_length_sets(B, T, rng)):
            calls = 2 + li % 2
            valid = R.valid_mask(B, T, lens)
            want, want_gx, data = None, [], []
            for _ in range(calls):
                x = rng.integers(-2, 3, (B, T, D0)).astype(np.float32)
                dz = rng.integers(-2, 3, (B, T)).astype(np.float32)
                big, grid = R.exactness_margin(params, x, L, 0.5, dz, lens=lens, calls=calls)
                assert big < 2 ** 20 and grid >= 2.0 ** -4, (big, grid)           # every f32 sum is exact in any order
                r = R.loss_and_grads(params, x, L, 0.5, lens=lens, dz=dz)
                g = R.pack({k: v for k, v in r["grads"].items()}, D0, H, L).astype(np.float64)
                want = g if want is None else want + g
                # a sum of zeros is +0 in the kernels' fma chains; numpy may return -0 for it (a column of -0 products): one sign of zero
                want_gx.append((r["grad_x"] + 0.0 if L else r["grad_x"]).astype(np.float32))
                x[~valid] = np.nan                                                 # never read past a length
                dz[~valid] = np.nan
                data.append((torch.from_numpy(x).to(_dev()), torch.from_numpy(dz).to(_dev())))
            lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=_dev())
            got = {}
            for seg, tr in trainers.items():
                tr.reset()
                for c, (xd, dzd) in enumerate(data):
                    pb = torch.full((B + 2, T + 3), -7.0, dtype=torch.float32, device=_dev())
                    gb = torch.full((B * T * D0 + 2 * PAD,), -7.0, dtype=torch.float32, device=_dev())
                    tr.grad(xd, lens=lens_d, dz=dzd, probs=(pb, pb[1].data_ptr(), T + 3), grad_x=(gb, gb.data_ptr() + 4 * PAD))
                    torch.cuda.synchronize()
                    gx = gb[PAD:PAD + B * T * D0].cpu().numpy().reshape(B, T, D0)
                    assert np.array_equal(_bits(gx), _bits(want_gx[c])), (B, T, li, seg, c)
                    assert not _bits(gx[~valid]).any()                             # +0 past the lengths
                    assert bool((gb[:PAD] == -7.0).all()) and bool((gb[PAD + B * T * D0:] == -7.0).all())
                    pn = pb.cpu().numpy()
                    inside = np.zeros((B + 2, T + 3), bool)
                    inside[1:B + 1, :T] = valid
                    assert (pn[~inside] == -7.0).all() and np.isfinite(pn[inside]).all() and ((pn[inside] >= 0) & (pn[inside] <= 1)).all()
                got[seg] = tr.read(_lib.HEAD_TRAIN_GRAD)
                assert np.array_equal(_bits(got[seg]), _bits((want + 0.0).astype(np.float32))), (B, T, li, seg)
                s = tr.read(_lib.HEAD_TRAIN_SCALARS)
                assert s["frames"] == calls * int(valid.sum()) and s["loss"] == 0.0 and s["t"] == 0
            assert got[32].tobytes() == got[64].tobytes() == got[0].tobytes()
    assert all(tr.canaries_intact() for tr in trainers.values())


# ------------------------------------------------------------------------------------------------ loss tier
@gpu
@pytest.mark.parametrize("B,T", [(2, 301), (3, 129)])
def test_loss_gradient_and_loss_sum_through_a_head_without_feed_forward_layers(B, T):
    from uvad_amd import _lib
    rng = np.random.default_rng(B * 1000 + T)
    D0 = 32
    params = {"classifier.weight": rng.standard_normal((1, D0)).astype(np.float32), "classifier.bias": np.array([0.25], np.float32)}
    rt, _ = _head_runtime(D0, 0, 0, 0.01, params)
    tr = Trainer(rt, segment=64)
    x = (rng.standard_normal((B, T, D0)) * 1.5).astype(np.float32)
    x[0, :8] *= 40.0                                                              # saturated frames among them
    y = rng.integers(0, 2, (B, T)).astype(np.uint8)
    fw = rng.uniform(0.25, 2.0, (B, T)).astype(np.float32)
    lens = [T, T // 3, 0][:B]
    valid = R.valid_mask(B, T, lens)
    n = int(valid.sum())
    xn, yn, fn = x.copy(), y.copy(), fw.copy()
    xn[~valid], yn[~valid], fn[~valid] = np.nan, 0xFF, np.nan
    to = lambda a: torch.from_numpy(a).to(_dev())
    lens_d = torch.tensor(lens, dtype=torch.int32, device=_dev())
    wc = params["classifier.weight"][0]
    for weights in (fn, None):
        tr.reset()
        pb = torch.full((B, T), -7.0, dtype=torch.float32, device=_dev())
        gb = torch.zeros((B, T, D0), dtype=torch.float32, device=_dev())
        tr.grad(to(xn), lens=lens_d, gt=to(yn), fw=None if weights is None else to(weights), probs=(pb, pb.data_ptr(), T), grad_x=(gb, gb.data_ptr()))
        torch.cuda.synchronize()
        p, gx = pb.cpu().numpy(), gb.cpu().numpy()
        assert (p[~valid] == -7.0).all()
        z64 = np.where(valid, np.nan_to_num(x).astype(np.float64) @ wc.astype(np.float64) + 0.25, 0.0)
        # z is a 32-term f32 chain ((D0 + 2) 2^-24 sum |x w| at the worst), a sigmoid's slope is at most 1 / 4, and its own evaluation a few ulp
        zerr = (D0 + 2) * 2.0 ** -24 * (np.abs(np.nan_to_num(x).astype(np.float64)) @ np.abs(wc.astype(np.float64)) + 0.25)
        with np.errstate(over="ignore"):
            assert (np.abs(p[valid] - 1.0 / (1.0 + np.exp(-z64[valid]))) <= zerr[valid] / 4 + 4 * 2.0 ** -24).all()
        w_valid = None if weights is None else np.where(valid, fw, 0).astype(np.float32)
        dz = np.where(valid, R.dz_f32(np.where(valid, p, 0.5), np.where(valid, y, 0), w_valid), 0).astype(np.float32)
        assert (dz[valid] == 0).any() and (dz[valid] != 0).sum() > n // 2          # saturated frames and ordinary ones
        assert np.array_equal(_bits(gx[valid]), _bits((dz[..., None] * wc[None, None, :]).astype(np.float32)[valid]))   # the dz the kernel used
        assert not _bits(gx[~valid]).any()
        g = R.unpack(tr.read(_lib.HEAD_TRAIN_GRAD), D0, 0, 0)
        dz64 = dz[valid].astype(np.float64)
        db_err = abs(float(g["classifier.bias"][0]) - dz64.sum())
        print(f"classifier.bias gradient: |err| {db_err:.3e}, bound {(n + 1) * 2.0 ** -24 * np.abs(dz64).sum():.3e}")
        assert db_err <= (n + 1) * 2.0 ** -24 * np.abs(dz64).sum()
        terms = R.bce_terms(p[valid], y[valid], None if weights is None else fw[valid])
        s = tr.read(_lib.HEAD_TRAIN_SCALARS)
        bound = 4 * n * 2.0 ** -53 * np.abs(terms).sum()
        print(f"loss sum {s['loss']:.12g}, float64 {terms.sum():.12g}, bound {bound:.3e}")
        assert s["frames"] == n and abs(s["loss"] - terms.sum()) <= bound
        head = tr.ws[(B, T)][PAD:PAD + 16].cpu().numpy()
        assert head[:8].view(np.float64)[0] == s["loss"] and int(head[8:].view(np.uint64)[0]) == n      # this call's sums in the workspace head
        if weights is None:                                                        # the scoring stage's loss on the same p and labels
            sc = rt.score_open(points=[(0.5, 1)])
            rt.score_step(sc, pb, to(np.where(valid, y, 0).astype(np.uint8)), lengths=lens_d)
            assert abs(rt.score_read(sc)["loss_sum"] - s["loss"]) <= bound
    assert tr.canaries_intact()


# ------------------------------------------------------------------------------------------------ shared: the seeded model and its taps
_SEEDED = {}


def _seeded(seed=0, shared=True):
    """The seeded PyanNet2 (4 x 128 bidirectional, head 128 / 2, slope 0.01) and real taps at B = 2, T = 301 with ragged lengths, frame
    weights and labels -- computed once per seed and left unchanged (shared=False: a model of the caller's own, which it may commit to)."""
    if shared and seed in _SEEDED:
        return _SEEDED[seed]
    import uvad_amd
    from uvad_amd.synth import seed_weights
    B, T = 2, 301
    m = uvad_amd.PyanNet2(encoding_dim=64)
    m.build()
    seed_weights(m, 1234 + seed, 2.0)
    m = m.to(_dev()).eval()
    rt = m.runtime(_dev())
    g = torch.Generator().manual_seed(50 + seed)
    feats = (torch.randn(B, T, 64, generator=g) * 2.0 - 3.0).to(_dev())
    lens = [T, 187]
    rt.classify(feats, lengths=lens)
    x0 = rt.taps(lin=False)[0].clone()
    torch.cuda.synchronize()
    x = x0.cpu().numpy()
    valid = R.valid_mask(B, T, lens)
    rng = np.random.default_rng(seed)
    y = (rng.random((B, T)) < 0.5).astype(np.uint8)
    assert 0.3 <= y[valid].mean() <= 0.7
    fw = rng.uniform(0.5, 1.5, (B, T)).astype(np.float32)
    params = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items() if k.startswith(("linear.", "classifier."))}
    out = dict(m=m, rt=rt, feats=feats, lens=lens, x0=x0, x=np.where(valid[..., None], x, 0).astype(np.float32), valid=valid, y=y, fw=fw,
               params=params, B=B, T=T)
    if shared:
        _SEEDED[seed] = out
    return out


def _torch_head(params, dtype):
    tp = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in params.items()}

    def fwd(x):
        out = x
        for l in range(2):
            out = torch.nn.functional.leaky_relu(torch.nn.functional.linear(out, tp[f"linear.{l}.weight"], tp[f"linear.{l}.bias"]), 0.01)
        return torch.sigmoid(torch.nn.functional.linear(out, tp["classifier.weight"], tp["classifier.bias"])).squeeze(-1)
    return tp, fwd


# ------------------------------------------------------------------------------------------------ accuracy tier
@gpu
def test_gradients_of_the_seeded_head_on_real_taps_within_four_times_torch_f32():
    """Per tensor, rms and max error against the float64 restatement divided by that tensor's float64 max-abs gradient, pooled over three
    seeds (rms: root of the mean square over the seeds; max: the largest), for the kernel and for torch.autograd in f32 on the CPU on the
    same inputs; the kernel may be at most 4 x torch."""
    from uvad_amd import _lib
    pool = {}
    for seed in range(3):
        s = _seeded(seed)
        ref = R.loss_and_grads(s["params"], s["x"], 2, 0.01, y=s["y"], w=s["fw"], lens=s["lens"])
        tr = Trainer(s["rt"])
        lens_d = torch.tensor(s["lens"], dtype=torch.int32, device=_dev())
        gb = torch.zeros_like(s["x0"])
        tr.grad(s["x0"], lens=lens_d, gt=torch.from_numpy(s["y"]).to(_dev()), fw=torch.from_numpy(s["fw"]).to(_dev()), grad_x=(gb, gb.data_ptr()))
        got = R.unpack(tr.read(_lib.HEAD_TRAIN_GRAD), 256, 128, 2)
        got["grad_x"] = gb.cpu().numpy()
        tp, fwd = _torch_head(s["params"], torch.float32)
        xt = torch.tensor(s["x"], requires_grad=True)
        v = torch.from_numpy(s["valid"])
        torch.nn.functional.binary_cross_entropy(fwd(xt)[v], torch.from_numpy(s["y"].astype(np.float32))[v], weight=torch.from_numpy(s["fw"])[v],
                                                 reduction="sum").backward()
        cpu = {k: t.grad.numpy() for k, t in tp.items()}
        cpu["grad_x"] = xt.grad.numpy()
        truth = dict(ref["grads"], grad_x=ref["grad_x"])
        for k, t in truth.items():
            scale = np.abs(t).max()
            for name, g in (("kernel", got[k]), ("torch", cpu[k])):
                e = np.abs(g.astype(np.float64).reshape(t.shape) - t) / scale
                pool.setdefault((k, name), []).append((float(np.sqrt((e ** 2).mean())), float(e.max())))
    worst = 0.0
    for k in truth:
        fig = {}
        for name in ("kernel", "torch"):
            a = np.array(pool[(k, name)])
            fig[name] = (float(np.sqrt((a[:, 0] ** 2).mean())), float(a[:, 1].max()))
        ratios = (fig["kernel"][0] / fig["torch"][0], fig["kernel"][1] / fig["torch"][1])
        worst = max(worst, *ratios)
        print(f"{k}: kernel rms {fig['kernel'][0]:.2e} max {fig['kernel'][1]:.2e} | torch f32 rms {fig['torch'][0]:.2e} max {fig['torch'][1]:.2e} | "
              f"ratios {ratios[0]:.2f} {ratios[1]:.2f}")
    assert worst <= 4.0, worst


# ------------------------------------------------------------------------------------------------ optimiser and trajectory
def _small_problem(seed=0, B=2, T=301, D0=64, H=32, L=2):
    rng = np.random.default_rng(seed)
    params = {k: (rng.uniform(-1, 1, shape) / np.sqrt(shape[-1] if len(shape) == 2 else H)).astype(np.float32) for k, shape in R.keys(D0, H, L)}
    x = np.tanh(rng.standard_normal((B, T, D0))).astype(np.float32)
    y = (x[..., :8].sum(-1) > 0).astype(np.uint8)
    return params, x, y


@gpu
def test_apply_equals_the_f32_adam_restatement_bit_for_bit():
    from uvad_amd import _lib
    D0, H, L = 64, 32, 2
    params, x, y = _small_problem()
    rt, _ = _head_runtime(D0, H, L, 0.01, params)
    hyper = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
    tr = Trainer(rt, **hyper)
    xd, yd = torch.from_numpy(x).to(_dev()), torch.from_numpy(y).to(_dev())
    lens_d = torch.tensor([301, 140], dtype=torch.int32, device=_dev())
    zero_d = torch.zeros(2, dtype=torch.int32, device=_dev())
    w, st = tr.read(_lib.HEAD_TRAIN_MASTERS), R.adam_init(tr.P)
    for step in range(7):
        for _ in range(1 + step % 2):                                             # one and two accumulated calls
            tr.grad(xd, lens=lens_d, gt=yd)
        acc, s = tr.read(_lib.HEAD_TRAIN_GRAD), tr.read(_lib.HEAD_TRAIN_SCALARS)
        assert s["frames"] == 441 * (1 + step % 2) and s["t"] == step and np.abs(acc).max() > 0
        tr.apply()
        w, st = R.adam_step(w, acc, s["frames"], st, lr=hyper["lr"], beta1=0.9, beta2=0.999, eps=1e-8)
        for which, want in ((_lib.HEAD_TRAIN_MASTERS, w), (_lib.HEAD_TRAIN_M, st["m"]), (_lib.HEAD_TRAIN_V, st["v"])):
            assert np.array_equal(_bits(tr.read(which)), _bits(want)), (step, which)
        s = tr.read(_lib.HEAD_TRAIN_SCALARS)
        assert s["t"] == step + 1 and s["frames"] == 0 and s["loss"] == 0.0 and not tr.read(_lib.HEAD_TRAIN_GRAD).any()
        assert _bits(s["bc1"]) == _bits(st["bc1"]) and _bits(s["bc2"]) == _bits(st["bc2"])
    before = bytes(tr.sbuf.cpu().numpy())
    tr.apply()                                                                    # nothing accumulated: no step
    tr.grad(xd, lens=zero_d, gt=yd)                                               # a call without a valid frame, then a step: still none
    tr.apply()
    assert bytes(tr.sbuf.cpu().numpy()) == before and tr.canaries_intact()


@gpu
def test_twenty_steps_track_the_float64_torch_loop_and_a_graph_replays_the_eager_bytes():
    s = _seeded(0)
    rt, B, T = s["rt"], s["B"], s["T"]
    rng = np.random.default_rng(5)
    u = rng.standard_normal(256)
    score = s["x"].astype(np.float64) @ u
    y = (score > np.median(score[s["valid"]])).astype(np.uint8)                   # labels the head can learn
    lens_d = torch.tensor(s["lens"], dtype=torch.int32, device=_dev())
    lr = 3e-3
    # float64 torch loop on the same taps and labels
    tp, fwd = _torch_head(s["params"], torch.float64)
    opt = torch.optim.Adam(list(tp.values()), lr=lr)
    xt, v = torch.tensor(s["x"], dtype=torch.float64), torch.from_numpy(s["valid"])
    want = []
    for _ in range(21):
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy(fwd(xt)[v], torch.from_numpy(y.astype(np.float64))[v])
        want.append(loss.item())
        loss.backward()
        opt.step()

    def run():
        h = rt.head_train_open(lr=lr)
        yd = torch.from_numpy(y).to(_dev())
        losses = []
        for _ in range(21):
            rt.head_train_grad(h, s["x0"], yd, lengths=lens_d)
            losses.append(rt.head_train_batch_loss(h).clone())
            rt.head_train_apply(h)
        torch.cuda.synchronize()
        return [float(l) for l in losses], bytes(h["state"].cpu().numpy())
    got, state_a = run()
    rel = [abs(a - b) / b for a, b in zip(got, want)]
    tp32, fwd32 = _torch_head(s["params"], torch.float32)                         # for the record only: the same loop in f32 on the CPU
    opt32, x32, y32, cpu32 = torch.optim.Adam(list(tp32.values()), lr=lr), torch.tensor(s["x"]), torch.from_numpy(y.astype(np.float32)), []
    for _ in range(21):
        opt32.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy(fwd32(x32)[v], y32[v])
        cpu32.append(loss.item())
        loss.backward()
        opt32.step()
    print(f"torch f32 CPU loop vs float64: worst relative {max(abs(a - b) / b for a, b in zip(cpu32, want)):.2e}")
    print("loss, kernel vs float64 torch loop:", [f"{a:.6f}/{b:.6f}" for a, b in zip(got[::5], want[::5])], f"worst relative {max(rel):.2e}")
    assert max(rel) <= 1e-3
    assert want[20] < 0.5 * want[0] and got[20] < 0.5 * got[0]
    _, state_b = run()
    assert state_a == state_b                                                     # two identical runs: the same bytes

    # ten steps, each one replay of ONE captured graph of grad + apply with new inputs copied in, against the eager run
    batches = []
    for k in range(10):
        xb = s["x0"] * (1.0 - 0.03 * k)
        batches.append((xb.contiguous(), torch.from_numpy(np.roll(y, k, axis=1).copy()).to(_dev()), torch.tensor([T - k, 150 + k], dtype=torch.int32, device=_dev())))
    he = rt.head_train_open(lr=lr)
    eager = []
    for xb, yb, lb in batches:
        rt.head_train_grad(he, xb, yb, lengths=lb)
        eager.append(rt.head_train_batch_loss(he).clone())
        rt.head_train_apply(he)
    hg = rt.head_train_open(lr=lr)
    sx, sy, sl = torch.zeros_like(s["x0"]), torch.zeros((B, T), dtype=torch.uint8, device=_dev()), torch.zeros(2, dtype=torch.int32, device=_dev())
    rt.head_train_grad(hg, sx, sy, lengths=sl)                                    # sizes the workspace; no valid frame, nothing accumulated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                 # one stream; a synchronisation or allocation would fail here
        rt.head_train_grad(hg, sx, sy, lengths=sl)
        rt.head_train_apply(hg)
    assert rt.head_train_read(hg)["step"] == 0                                    # captured, not run
    replayed = []
    for xb, yb, lb in batches:
        sx.copy_(xb), sy.copy_(yb), sl.copy_(lb)
        graph.replay()
        replayed.append(rt.head_train_batch_loss(hg).clone())
    torch.cuda.synchronize()
    assert [float(a) for a in eager] == [float(b) for b in replayed]
    assert bytes(he["state"].cpu().numpy()) == bytes(hg["state"].cpu().numpy())
    assert rt.head_train_read(hg)["step"] == 10


# ------------------------------------------------------------------------------------------------ commit and host layer
@gpu
def test_commit_serves_the_adapted_head_and_leaves_the_encoder_and_other_contexts_alone():
    import uvad_amd
    s = _seeded(7, shared=False)
    m, rt, feats = s["m"], s["rt"], s["feats"]
    other = uvad_amd.VadRuntime(_dev(), model={"encoding_dim": 64, "lstm": m.hparams.lstm, "linear": m.hparams.linear})
    other.load_state_dict(m.state_dict())                                         # finalized earlier with the original weights
    assert rt.weights_shared_by() == 2 == other.weights_shared_by()
    lg0, _ = rt.classify(feats)
    lg0, tap0 = lg0.clone(), rt.taps(lin=False)[0].clone()
    h = rt.head_train_open(lr=1e-2)
    yd = torch.from_numpy(s["y"]).to(_dev())
    for _ in range(3):
        rt.head_train_grad(h, tap0, yd)
        rt.head_train_apply(h)
    rt.head_train_commit(h)
    assert rt.weights_shared_by() == 1 == other.weights_shared_by()               # the shared upload block split
    lg1, _ = rt.classify(feats)
    tap1 = rt.taps(lin=False)[0]
    probs, _ = rt.head_train_grad(h, tap0, yd, want_probs=True)                   # the trainer's own forward with the committed masters
    torch.cuda.synchronize()
    assert torch.equal(tap0, tap1)                                                # the encoder is frozen
    p = probs.cpu().numpy().astype(np.float64)
    ok = (p > 0) & (p < 1)
    z = np.log(p[ok] / (1.0 - p[ok]))
    tol = 1e-4 + 2.0 ** -24 / (p[ok] * (1.0 - p[ok]))                             # the standing logit bound, and p's own f32 rounding seen through the logit
    lg1n = lg1.cpu().numpy().astype(np.float64)
    assert ok.mean() > 0.9 and (np.abs(lg1n[ok] - z) <= tol).all()
    assert float((lg1 - lg0).abs().max()) > 1e-2                                  # and it is another head than before
    lgo, _ = other.classify(feats)
    assert torch.equal(lgo, lg0)
    sd = rt.head_train_state_dict(h)
    assert list(sd) == [k for k, _ in R.keys(256, 128, 2)] and not torch.equal(sd["linear.0.weight"], m.state_dict()["linear.0.weight"].cpu())
    other.close()


@gpu
def test_vadmodel_adapt_head_step_commit_and_checkpoint_round_trip(tmp_path):
    from uvad_amd.engine import VadModel
    from uvad_amd.synth import seed_weights
    md = {"encoding_dim": 64, "lstm": {"num_layers": 2}}
    vm = VadModel("PyanNet2", md, learning_rate=3e-3)
    seed_weights(vm.model, 77, 2.0)
    vm = vm.to(_dev()).eval()
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(2, 129, 64, generator=g) * 2.0 - 3.0).to(_dev())
    y = (torch.rand(2, 129, generator=g) < 0.5).to(torch.uint8)
    batch = {"inputs": x, "is_voice": y, "lengths": [129, 77]}
    with pytest.raises(NotImplementedError):
        vm.training_step({}, 0)
    with pytest.raises(NotImplementedError):
        vm.configure_optimizers()
    cached = dict(batch, lstm_out=vm.lstm_out(batch).clone())
    vm2 = VadModel("PyanNet2", md, learning_rate=3e-3)
    vm2.load_state_dict(vm.state_dict())
    vm2 = vm2.to(_dev()).eval()
    la = [vm.adapt_head_step(batch, i, accumulate=2) for i in range(4)]
    lb = [vm2.adapt_head_step(cached, i, accumulate=2) for i in range(4)]
    assert all(t.is_cuda and t.dim() == 0 for t in la)
    torch.cuda.synchronize()
    assert [float(t) for t in la] == [float(t) for t in lb]                        # cached taps: the same bits
    assert float(la[1]) == float(la[0]) and float(la[2]) < float(la[0])            # a step after every second call
    before = {k: v.clone() for k, v in vm.state_dict().items()}
    vm.adapt_head_commit()
    vm2.adapt_head_commit()
    after = vm.state_dict()
    for k in before:
        changed = not torch.equal(before[k], after[k])
        assert changed == k.startswith(("model.linear.", "model.classifier.")), k
        assert torch.equal(after[k], vm2.state_dict()[k])
    path = os.path.join(tmp_path, "adapted.ckpt")
    torch.save({"state_dict": vm.state_dict()}, path)
    back = VadModel.load_from_checkpoint(path, model_name="PyanNet2", model_dict=md).to(_dev()).eval()
    assert torch.equal(back(x), vm(x))
    assert vm.model._rt_stamp == vm.model._stamp(_dev())                          # the committed runtime is served as it is: no second upload


@gpu
def test_a_sincnet_context_goes_through_grad_apply_and_commit():
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet(lstm={"num_layers": 1}, linear={"hidden_size": 64, "num_layers": 1})
    m.build()
    seed_weights(m, 21, 2.0)
    m = m.to(_dev()).eval()
    rt = m.runtime(_dev())
    wav = torch.randn(2, 16000, generator=torch.Generator().manual_seed(2)).to(_dev()) * 0.1
    feats = rt.sincnet(wav)
    lg0, _ = rt.classify(feats)
    lg0, x0 = lg0.clone(), rt.taps(lin=False)[0].clone()
    B, T = lg0.shape
    y = torch.from_numpy((np.random.default_rng(0).random((B, T)) < 0.5).astype(np.uint8)).to(_dev())
    h = rt.head_train_open(lr=1e-2)
    rt.head_train_grad(h, x0, y)
    rt.head_train_apply(h)
    assert rt.head_train_read(h)["step"] == 1
    rt.head_train_commit(h)
    lg1, _ = m.forward_logits(wav)
    assert torch.isfinite(lg1).all() and float((lg1 - lg0).abs().max()) > 1e-3


@gpu
def test_adapt_vad_and_main_lower_the_validation_loss_on_two_synthetic_files(tmp_path):
    import wave
    import main as entry
    from config.config import load_config
    from src.scripts import adapt_vad
    from uvad_amd.engine import VadModel
    from uvad_amd.synth import synth_pcm
    paths, labels = [], []
    for k, secs in enumerate((3.0, 4.1)):
        x = synth_pcm(1, int(secs * 16000), seed=900 + k)[0]
        x[int(1.0 * 16000):int(2.0 * 16000)] *= 0.02                               # a quiet second in the middle: the non-speech
        p, f = tmp_path / f"a{k}.wav", tmp_path / f"a{k}.txt"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
        f.write_text(f"0.0\t1.0\tSPC\n2.0\t{secs}\tSPC\n")
        paths.append(str(p)); labels.append(str(f))
    cfg = load_config()
    cfg.model_dict.encoding_dim = 64
    cfg.model_dict.lstm = {"num_layers": 2}
    cfg.weights_scale = 2.0
    cfg.input.kind, cfg.input.paths, cfg.input.labels = "wav", paths, labels
    cfg.function, cfg.learning_rate, cfg.max_epochs, cfg.check_val_every_n_epoch = "adapt", 3e-3, 6, 3
    cfg.adapted_checkpoint_path = str(tmp_path / "out" / "adapted.ckpt")
    got = entry.main(cfg)
    assert [e for e, _ in got["val_loss"]] == [0, 3, 6] and len(got["train_loss"]) == 6
    assert got["val_loss"][-1][1] < got["val_loss"][0][1] and got["train_loss"][-1] < got["train_loss"][0]
    assert "val_detection_error_rate" in got["val_metrics"]
    vm = VadModel.load_from_checkpoint(got["checkpoint_path"], model_name="PyanNet2", model_dict=dict(cfg.model_dict))
    blob = torch.load(got["checkpoint_path"], weights_only=True)
    assert blob["epoch"] == 6 and blob["global_step"] == 12 and all(k.startswith("model.") for k in blob["state_dict"])
    cfg.accumulate_grad_batches, cfg.input.val_paths, cfg.input.val_labels = 2, paths[:1], labels[:1]
    again = adapt_vad(**cfg)
    assert again["val_loss"][-1][1] < again["val_loss"][0][1] and vm is not None
