"""Dropout between the trainable LSTM layers on the device (uvad_lstm_train_set_dropout, uvad_dropout_apply, include/uvad.h) against
tests/lstm_dropout_ref.py and torch on the CPU.

  the mask          uvad_dropout_apply byte for byte: -0, NaN and Inf at dropped positions come out +0, in place, canaries
  p = 0             a context switched on and off again equals one never switched: outputs, gradients, every state byte, the count
  accuracy          d_y, d_grad_in and every gradient against the float64 restatement with the same (seed, draw), over the float64 tensor's
                    max-abs, three seeds pooled: at most 4 x the error of the torch-f32 comparator with the same masks
  draw ordinal      one mask per forward call, the backward call's mask from the workspace it is given, a changed setting in between
  lengths, guard    NaN past the lengths reaches nothing; a mismatched workspace header leaves everything untouched
  graphs            a captured step draws a fresh mask per replay and lands on the eager bytes
  twenty steps      the losses track the float64 torch loop with the same masks within 4 x torch's own f32 loop
  host              lstm_train_open(dropout=), adapt_step(dropout=), train_step, train_vad, main(function = "train")
"""
import ctypes as C

import numpy as np
import pytest
import torch

import head_train_ref as HR
import lstm_dropout_ref as DR
import lstm_train_ref as R
import test_gpu_lstm_train as T0      # its Trainer (the C entry points on buffers with canaries) and helpers, not its tests

gpu = pytest.mark.gpu
PAD = T0.PAD
_bits, _dev, _to, _lens_d = T0._bits, T0._dev, T0._to, T0._lens_d

# B 5: two recurrence tiles, one partly empty; lengths with 0, 1 and T; H 64 x 2 directions x 3 layers: two boundaries with different k
B, T, DIN = 5, 19, 16
LENS = [19, 0, 7, 19, 1]
SHAPES = [(64, 2, 3), (128, 1, 2)]    # (H, dirs, layers)
SEED = 0x5EED0123456789AB


class Trainer(T0.Trainer):
    """T0.Trainer with the dropout setting re-asserted after every configure, as the runtime does.  drop = None: never set."""
    drop = None

    def configure(self):
        super().configure()
        if self.drop is not None:
            self.rt._check(self.lib.uvad_lstm_train_set_dropout(self.rt.ctx, self.drop[0], self.drop[1]))

    def draws(self):
        return int(self.sbuf[PAD + 56:PAD + 64].cpu().numpy().view(np.uint64)[0])

    def grads(self, shape):
        return R.unpack(self.grad(), *shape)


_SHARED = {}


def _problem(H, dirs, layers, seed=0):
    """Runtime, parameters and inputs of one configuration: built once, shared by the tests and left unchanged."""
    key = (H, dirs, layers, seed)
    if key not in _SHARED:
        shape = (DIN, H, dirs, layers, 0)
        params, x, dy = R.seeded(300 + seed + H + layers, *shape, B, T, scale=2.0)
        rt, _, _ = T0._runtime(DIN, H, dirs, layers, params)
        valid = HR.valid_mask(B, T, LENS)
        xd, dd = T0._poisoned(x, dy, valid)                                       # NaN past the lengths
        _SHARED[key] = dict(rt=rt, params=params, x=x, dy=dy, shape=shape, valid=valid, xd=xd, dd=dd, ref={})
    return _SHARED[key]


def _ref(p, draw, prob, seed=SEED):
    """The float64 restatement of one configuration at (seed, draw, p): computed once."""
    key = (draw, float(np.float32(prob)), seed)
    if key not in p["ref"]:
        _, H, dirs, layers, _ = p["shape"]
        p["ref"][key] = DR.forward_backward(p["params"], p["x"], p["dy"], H, dirs, layers, 0, LENS, seed=seed, draw=draw, p=prob)
    return p["ref"][key]


def _close(a, b, tol=1e-4):
    a, b = np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * np.abs(b).max()


# ------------------------------------------------------------------------------------------------ the mask, to the bit
@gpu
@pytest.mark.parametrize("cols", [4, 128, 2048])
@pytest.mark.parametrize("rows", [1, 95])
def test_dropout_apply_equals_the_restatement_byte_for_byte(rows, cols):
    from uvad_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(rows + cols)
    for prob in (0.0, np.float32(0.3), 0.5, np.nextafter(np.float32(1), np.float32(0))):
        for layer, draw in ((0, 0), (2, 1), (65535, (1 << 40) + 3)):
            x = rng.standard_normal((rows, cols)).astype(np.float32)
            keep = DR.mask(SEED, draw, layer, rows, cols, prob)
            dropped = np.argwhere(~keep)
            for k, v in enumerate((-0.0, np.nan, np.inf, -np.inf)):               # at positions the restatement says are dropped
                for r, c in dropped[k::4][:8]:
                    x[r, c] = v
            x.flat[rng.integers(0, x.size, 3)] = -0.0                             # ... and -0 anywhere: kept, it stays -0
            want = DR.apply_f32(x, SEED, draw, layer, prob)
            assert not _bits(want[~keep]).any() and (prob != 0.0 or want.tobytes() == x.tobytes())
            n = rows * cols
            src = torch.full((n + 2 * PAD,), -7.0, dtype=torch.float32, device=_dev())
            dst = torch.full((n + 2 * PAD,), -7.0, dtype=torch.float32, device=_dev())
            src[PAD:PAD + n] = _to(x).reshape(-1)
            call = lambda a, b: lib.uvad_dropout_apply(C.c_void_p(a.data_ptr() + 4 * PAD), C.c_void_p(b.data_ptr() + 4 * PAD), rows, cols, layer, draw,
                                                       float(prob), SEED, None)
            assert call(src, dst) == 0
            torch.cuda.synchronize()
            assert dst[PAD:PAD + n].cpu().numpy().tobytes() == want.tobytes(), (float(prob), layer, draw)
            assert src[PAD:PAD + n].cpu().numpy().tobytes() == x.tobytes()        # out of place: the input is left alone
            assert call(src, src) == 0                                            # in place: the same bytes
            torch.cuda.synchronize()
            assert src[PAD:PAD + n].cpu().numpy().tobytes() == want.tobytes()
            for b in (src, dst):
                assert bool((b[:PAD] == -7.0).all()) and bool((b[PAD + n:] == -7.0).all())


# ------------------------------------------------------------------------------------------------ p = 0 is the code without the stage
@gpu
@pytest.mark.parametrize("H,dirs,layers", SHAPES)
def test_switched_on_and_off_again_equals_never_switched(H, dirs, layers):
    p = _problem(H, dirs, layers)
    ld = _lens_d(LENS)
    never = Trainer(p["rt"])
    y0 = never.forward(p["xd"], ld)
    g0 = never.backward(p["xd"], p["dd"], ld)
    rt2, _, _ = T0._runtime(DIN, H, dirs, layers, p["params"])
    tr = Trainer(rt2)
    tr.drop = (0.5, SEED)
    tr.configure()
    tr.drop = (0.0, SEED)
    y1 = tr.forward(p["xd"], ld)
    g1 = tr.backward(p["xd"], p["dd"], ld)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(g0, g1) and bool(y0.any()) and bool(g0.any())
    assert bytes(never.sbuf.cpu().numpy()) == bytes(tr.sbuf.cpu().numpy())
    assert tr.draws() == 0 and never.draws() == 0
    assert never.canaries_intact() and tr.canaries_intact()
    rt2.close()


# ------------------------------------------------------------------------------------------------ accuracy with the mask on
@gpu
@pytest.mark.parametrize("H,dirs,layers", SHAPES)
@pytest.mark.parametrize("prob", [0.5, 0.3])
def test_output_and_gradients_within_four_times_the_torch_f32_comparator(H, dirs, layers, prob):
    """Per tensor, rms and max error against the float64 restatement over that tensor's float64 max-abs, pooled over three seeds, for the
    kernels and for the stacked one-layer nn.LSTMs in f32 on the CPU with the same masks; the kernels may be at most 4 x torch (DESIGN.md
    3.26's bound).  A wrong mask, a missing scale or a backward pass under another mask is off by orders of magnitude."""
    pool = {}
    for seed in range(3):
        p = _problem(H, dirs, layers, seed)
        tr = Trainer(p["rt"], segment=32)
        tr.drop = (prob, SEED + seed)
        y = tr.forward(p["xd"], _lens_d(LENS))
        gin = tr.backward(p["xd"], p["dd"], _lens_d(LENS))
        got = dict(tr.grads(p["shape"]), y=y.cpu().numpy(), grad_in=gin.cpu().numpy())
        assert tr.canaries_intact() and tr.draws() == 1
        truth = _ref(p, 0, prob, SEED + seed)
        cpu = DR.torch_forward_backward(p["params"], p["x"], p["dy"], H, dirs, layers, 0, LENS, seed=SEED + seed, draw=0, p=prob, dtype=torch.float32)
        for k in ["y", "grad_in"] + list(truth["grads"]):
            t, c = (truth[k], cpu[k]) if k in truth else (truth["grads"][k], cpu["grads"][k])
            for who, a in (("kernel", got[k]), ("torch", c)):
                e = np.abs(np.asarray(a, np.float64).reshape(t.shape) - t) / np.abs(t).max()
                pool.setdefault((k, who), []).append((float((e ** 2).mean()), float(e.max())))
    worst = 0.0
    for k in sorted({k for k, _ in pool}):
        f = {who: (np.sqrt(np.mean([v[0] for v in pool[k, who]])), max(v[1] for v in pool[k, who])) for who in ("kernel", "torch")}
        ratios = (f["kernel"][0] / f["torch"][0], f["kernel"][1] / f["torch"][1])
        worst = max(worst, *ratios)
        print(f"{k}: kernel rms {f['kernel'][0]:.2e} max {f['kernel'][1]:.2e} | torch f32 rms {f['torch'][0]:.2e} max {f['torch'][1]:.2e} | "
              f"ratios {ratios[0]:.2f} {ratios[1]:.2f}")
    print(f"H {H} dirs {dirs} layers {layers} p {prob}: worst ratio {worst:.2f}")
    assert worst <= 4.0


# ------------------------------------------------------------------------------------------------ the draw ordinal
@gpu
@pytest.mark.parametrize("H,dirs,layers", SHAPES)
def test_each_forward_call_draws_its_own_mask_and_backward_uses_its_workspace_record(H, dirs, layers):
    p = _problem(H, dirs, layers)
    ld = _lens_d(LENS)
    tr = Trainer(p["rt"])
    tr.drop = (0.5, SEED)
    ya = tr.forward(p["xd"], ld, ws_key="a").clone()
    yb = tr.forward(p["xd"], ld, ws_key="b").clone()
    torch.cuda.synchronize()
    assert tr.draws() == 2 and not torch.equal(ya, yb)
    r0, r1 = _ref(p, 0, 0.5), _ref(p, 1, 0.5)
    assert _close(ya.cpu().numpy(), r0["y"]) and _close(yb.cpu().numpy(), r1["y"]) and not _close(ya.cpu().numpy(), r1["y"], 1e-2)
    gin = tr.backward(p["xd"], p["dd"], ld, ws_key="a")                           # A's record: draw 0, though B's forward call came later
    g = tr.grads(p["shape"])
    assert _close(gin.cpu().numpy(), r0["grad_in"]) and all(_close(g[k], r0["grads"][k]) for k in g)
    assert not _close(gin.cpu().numpy(), r1["grad_in"], 1e-2)
    # a setting changed between a forward call and its backward call changes no byte of the backward call's result
    runs = []
    for change in (None, (np.float32(0.3), SEED ^ 0xFFFF)):
        tr.drop = (0.5, SEED)
        tr.reset()
        tr.forward(p["xd"], ld, ws_key="a")
        if change:
            tr.drop = change
        gi = tr.backward(p["xd"], p["dd"], ld, ws_key="a")
        torch.cuda.synchronize()
        runs.append((gi.cpu().numpy().tobytes(), bytes(tr.sbuf.cpu().numpy())))
    assert runs[0] == runs[1] and _close(np.frombuffer(runs[0][0], np.float32), r0["grad_in"].reshape(-1))
    assert tr.canaries_intact()


# ------------------------------------------------------------------------------------------------ lengths and the workspace guard
@gpu
@pytest.mark.parametrize("H,dirs,layers", SHAPES)
def test_nan_past_the_lengths_reaches_nothing_and_a_mismatched_workspace_writes_nothing(H, dirs, layers):
    p = _problem(H, dirs, layers)
    ld, valid = _lens_d(LENS), p["valid"]
    tr = Trainer(p["rt"])
    tr.drop = (0.5, SEED)
    y = tr.forward(p["xd"], ld, ws_key="w")
    gin = tr.backward(p["xd"], p["dd"], ld, ws_key="w")
    torch.cuda.synchronize()
    y, gin, g = y.cpu().numpy(), gin.cpu().numpy(), tr.grad()
    assert not _bits(y[~valid]).any() and not _bits(gin[~valid]).any()            # +0 past the lengths
    assert np.isfinite(y).all() and np.isfinite(gin).all() and np.isfinite(g).all() and np.abs(g).max() > 0
    before, ws_before = bytes(tr.sbuf.cpu().numpy()), bytes(tr.ws["w"].cpu().numpy())
    xs, ds = p["xd"].reshape(T, B, DIN), p["dd"].reshape(T, B, H * dirs)          # B and T swapped: the same workspace size, another header
    gs = tr.backward(xs, ds, ws_key="w")                                          # (no lengths: the set above has B entries)
    torch.cuda.synchronize()
    assert bytes(tr.sbuf.cpu().numpy()) == before and bytes(tr.ws["w"].cpu().numpy()) == ws_before
    assert bool((gs == -7.0).all()) and tr.canaries_intact()


# ------------------------------------------------------------------------------------------------ determinism and graphs
@gpu
def test_same_seed_same_bytes_other_seed_other_bytes():
    H, dirs, layers = SHAPES[0]
    p = _problem(H, dirs, layers)
    ld = _lens_d(LENS)
    runs = []
    for seed in (SEED, SEED, SEED + 1):
        tr = Trainer(p["rt"])
        tr.drop = (0.5, seed)
        y = tr.forward(p["xd"], ld)
        gin = tr.backward(p["xd"], p["dd"], ld)
        torch.cuda.synchronize()
        runs.append((y.cpu().numpy().tobytes(), gin.cpu().numpy().tobytes(), bytes(tr.sbuf.cpu().numpy())))
    assert runs[0] == runs[1] and all(a != b for a, b in zip(runs[0], runs[2]))


@gpu
def test_a_captured_step_draws_a_fresh_mask_per_replay_and_lands_on_the_eager_bytes():
    H, dirs, layers, lr = 64, 2, 3, 3e-3
    rt, _, _ = T0._runtime(DIN, H, dirs, layers, seed=9, scale=2.0)
    rng = np.random.default_rng(2)
    batches = []
    for k in range(3):
        x = rng.standard_normal((B, T, DIN)).astype(np.float32)
        batches.append((_to(x), _to((x[..., :8].sum(-1) > 0).astype(np.uint8)), _lens_d([T - k, 0, 7 + k, T, 1])))

    def step(hh, hl, x, y, n):
        out = rt.lstm_train_forward(hl, x, lengths=n)
        _, gx = rt.head_train_grad(hh, out, y, lengths=n, want_grad_x=True)
        rt.lstm_train_backward(hl, x, gx, lengths=n)
        rt.head_train_apply(hh)
        rt.lstm_train_apply(hl)

    def reset(hl):
        rt._lstm_train_configure(hl)
        rt._check(rt.lib.uvad_lstm_train_reset(rt.ctx, hl["state"].data_ptr(), hl["state"].numel(), None))
    sx, sy, sl = torch.zeros_like(batches[0][0]), torch.zeros((B, T), dtype=torch.uint8, device=_dev()), torch.zeros(B, dtype=torch.int32, device=_dev())
    states = []
    for graphed in (False, True):
        hh, hl = rt.head_train_open(lr=lr), rt.lstm_train_open(layers=layers, lr=lr, dropout=0.5, seed=SEED)
        step(hh, hl, sx, sy, sl)                                                  # sizes the workspaces: no valid frame, but one mask drawn
        torch.cuda.synchronize()
        assert rt.lstm_train_draws(hl) == 1
        reset(hl)                                                                 # both runs start from the same reset
        if graphed:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step(hh, hl, sx, sy, sl)
            assert rt.lstm_train_draws(hl) == 0                                   # captured, not run
        for x, y, n in batches:
            if graphed:
                sx.copy_(x), sy.copy_(y), sl.copy_(n)
                graph.replay()
            else:
                step(hh, hl, x, y, n)
        torch.cuda.synchronize()
        assert rt.lstm_train_draws(hl) == 3 and rt.lstm_train_read(hl)["step"] == 3
        states.append((bytes(hl["state"].cpu().numpy()), bytes(hh["state"].cpu().numpy())))
    assert states[0] == states[1]
    rt.close()


# ------------------------------------------------------------------------------------------------ twenty Adam steps
def _torch_model(sd, H, layers, dtype):
    """The seeded bidirectional stack as one-layer nn.LSTMs with the head 32 / 1 on the CPU -> (parameters, forward(x, lens, factors) -> p (B, T))."""
    params = {k: v.numpy() for k, v in sd.items() if k.startswith("lstm.")}
    stack = DR.torch_layers(params, DIN, H, 2, layers, 0, dtype)
    head = {k: sd[k].detach().clone().to(dtype).requires_grad_(True) for k in ("linear.0.weight", "linear.0.bias", "classifier.weight", "classifier.bias")}

    def fwd(x, lens, factors):
        out = DR.torch_stack(stack, x, torch.tensor(lens), factors, 0)
        out = torch.nn.functional.leaky_relu(torch.nn.functional.linear(out, head["linear.0.weight"], head["linear.0.bias"]), 0.01)
        return torch.sigmoid(torch.nn.functional.linear(out, head["classifier.weight"], head["classifier.bias"])).squeeze(-1)
    return [q for m in stack for q in m.parameters()] + list(head.values()), fwd


@gpu
def test_twenty_steps_with_dropout_track_the_float64_torch_loop_with_the_same_masks():
    """H 64, two bidirectional layers, head 32 / 1, B 4, T 37, ragged, p = 0.3: the rms deviation of the 20 losses from the float64 torch
    loop under the same masks (draw = the step), pooled over three seeds, at most 4 x the deviation of torch's own f32 loop."""
    H, layers, Bt, Tt, lr, prob = 64, 2, 4, 37, 3e-3, np.float32(0.3)
    lens = [37, 21, 9, 30]
    v = torch.from_numpy(HR.valid_mask(Bt, Tt, lens))
    dev2 = {"kernel": [], "torch": []}
    for seed in range(3):
        rt, sd, _ = T0._runtime(DIN, H, 2, layers, seed=40 + seed, scale=2.0)
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((Bt, Tt, DIN)).astype(np.float32)
        y = (x[..., :8].sum(-1) > 0).astype(np.uint8)
        masks = [DR.mask(SEED + seed, step, 0, Bt * Tt, 2 * H, prob).reshape(Bt, Tt, 2 * H) for step in range(20)]
        loops = {}
        for dtype in (torch.float64, torch.float32):
            prm, fwd = _torch_model(sd, H, layers, dtype)
            opt = torch.optim.Adam(prm, lr=lr)
            xt, yt, losses = torch.tensor(x, dtype=dtype), torch.from_numpy(y).to(dtype), []
            sc = torch.tensor(float(DR.scale(prob)), dtype=dtype)
            for step in range(20):
                opt.zero_grad()
                loss = torch.nn.functional.binary_cross_entropy(fwd(xt, lens, {0: torch.from_numpy(masks[step]).to(dtype) * sc})[v], yt[v])
                losses.append(loss.item())
                loss.backward()
                opt.step()
            loops[dtype] = np.array(losses)
        hh, hl = rt.head_train_open(lr=lr), rt.lstm_train_open(layers=layers, lr=lr, dropout=float(prob), seed=SEED + seed)
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
        assert rt.lstm_train_read(hl)["step"] == 20 and rt.lstm_train_draws(hl) == 20
        rt.close()
    k, t = (float(np.sqrt(np.mean(dev2[w]))) for w in ("kernel", "torch"))
    print(f"rms deviation of 20 losses from the float64 loop, three seeds: kernel {k:.3e}, torch f32 {t:.3e}, ratio {k / t:.2f}")
    assert k <= 4.0 * t


# ------------------------------------------------------------------------------------------------ host layer
@gpu
def test_lstm_train_open_and_adapt_step_hand_the_setting_to_the_device():
    from uvad_amd.engine import VadModel
    H, dirs, layers = SHAPES[0]
    p = _problem(H, dirs, layers)
    rt, ld = p["rt"], _lens_d(LENS)
    hl = rt.lstm_train_open(layers=layers, dropout=0.5, seed=SEED)
    other = rt.lstm_train_open(layers=layers)                                     # a second handle on the context, without dropout
    y = rt.lstm_train_forward(hl, p["xd"], lengths=ld).clone()
    y_plain = rt.lstm_train_forward(other, p["xd"], lengths=ld).clone()
    y2 = rt.lstm_train_forward(hl, p["xd"], lengths=ld).clone()                   # the handle re-asserts its setting
    torch.cuda.synchronize()
    assert rt.lstm_train_draws(hl) == 2 and rt.lstm_train_draws(other) == 0
    assert _close(y.cpu().numpy(), _ref(p, 0, 0.5)["y"]) and _close(y2.cpu().numpy(), _ref(p, 1, 0.5)["y"])
    assert _close(y_plain.cpu().numpy(), R.forward(p["params"], p["x"], H, dirs, layers, 0, LENS)[0])
    with pytest.raises(ValueError):
        rt.lstm_train_open(layers=layers, dropout=1.0)
    xx = _to(p["x"])
    got = rt.dropout_apply(xx, 2, 5, 0.5, SEED)
    assert got.cpu().numpy().tobytes() == DR.apply_f32(p["x"].reshape(B * T, DIN), SEED, 5, 2, 0.5).tobytes()
    assert rt.dropout_apply(xx, 2, 5, 0.5, SEED, out=xx) is xx and torch.equal(xx, got)

    md = {"encoding_dim": DIN, "lstm": {"hidden_size": H, "num_layers": layers, "bidirectional": dirs == 2, "dropout": 0.5},
          "linear": {"hidden_size": 32, "num_layers": 1}}
    vm = VadModel("PyanNet2", md, learning_rate=3e-3)
    assert vm.model.train_dropout == 0.5
    vm.model.load_state_dict({k: torch.from_numpy(v) for k, v in p["params"].items()}, strict=False)
    vm = vm.to(_dev()).eval()
    batch = {"inputs": _to(p["x"]), "is_voice": torch.zeros(B, T, dtype=torch.uint8), "lengths": LENS}
    loss = vm.adapt_step(batch, 0, lstm_layers=layers, dropout=0.5, seed=SEED)
    held = vm._adapt_full
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and held[0].lstm_train_draws(held[2]) == 1
    assert _close(held[2]["_keep"][2].cpu().numpy(), _ref(p, 0, 0.5)["y"])        # the forward output of that step: mask (SEED, draw 0)
    vm.adapt_step(batch, 1, lstm_layers=layers)                                   # dropout None: today's step, no mask drawn
    torch.cuda.synchronize()
    assert held[0].lstm_train_draws(held[2]) == 1
    torch.manual_seed(SEED & 0x7FFFFFFF)
    vm.train_step(batch, 2)                                                       # every layer, the model's dropout, torch's seed
    torch.cuda.synchronize()
    assert vm._adapt_full is held and held[2]["dropout"] == 0.5 and held[2]["seed"] == SEED & 0x7FFFFFFF
    assert held[0].lstm_train_draws(held[2]) == 2
    vm.train_commit()
    with pytest.raises(NotImplementedError):
        vm.training_step({}, 0)
    with pytest.raises(NotImplementedError):
        vm.configure_optimizers()
    with pytest.raises(NotImplementedError, match="SincNet"):
        VadModel("PyanNet", {}).train_step(batch, 0)


@gpu
def test_train_vad_trains_every_layer_from_initialisation_and_writes_its_checkpoint(tmp_path):
    import wave
    import main as entry
    from config.config import load_config
    from uvad_amd.engine import VadModel
    from uvad_amd.synth import synth_pcm
    paths, labels = [], []
    for k, secs in enumerate((3.2, 2.5)):
        x = synth_pcm(1, int(secs * 16000), seed=900 + k)[0]
        x[int(0.5 * 16000):int(1.0 * 16000)] *= 0.02
        x[int(1.8 * 16000):int(2.3 * 16000)] *= 0.02
        p, f = tmp_path / f"a{k}.wav", tmp_path / f"a{k}.txt"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
        f.write_text(f"0.0\t0.5\tSPC\n1.0\t1.8\tSPC\n2.3\t{secs}\tSPC\n")
        paths.append(str(p)); labels.append(str(f))

    def config(dropout, where):
        cfg = load_config()
        cfg.model_dict.encoding_dim = 64
        cfg.model_dict.lstm = {"hidden_size": 64, "num_layers": 2, "dropout": dropout}
        cfg.model_dict.linear = {"hidden_size": 32, "num_layers": 1}
        cfg.input.kind, cfg.input.paths, cfg.input.labels = "wav", paths, labels
        cfg.function, cfg.learning_rate, cfg.max_epochs, cfg.check_val_every_n_epoch = "train", 1e-2, 3, 2
        cfg.window_seconds, cfg.max_duration, cfg.accumulate_grad_batches = 1.0, 2.0, 2
        cfg.experiments_dir = str(tmp_path / where)
        return cfg
    from uvad_amd.scripts import train_vad
    cfg = config(0.0, "plain")
    got = train_vad(**cfg)
    # 4 + 3 windows of one second (the tails 0.2 and 0.5 s kept as shorter rows), two rows per batch: 4 batches per epoch
    assert got["global_step"] == 4 * 3 // 2 and [e for e, _ in got["val_loss"]] == [2, 3]
    assert len(got["train_loss"]) == 3 and np.isfinite(got["train_loss"]).all() and np.isfinite([l for _, l in got["val_loss"]]).all()
    assert got["train_loss"][2] < got["train_loss"][0]
    assert got["checkpoint_path"] == str(tmp_path / "plain" / "checkpoint-epoch=03.ckpt")
    md = dict(cfg.model_dict)
    vm = VadModel.load_from_checkpoint(got["checkpoint_path"], model_name="PyanNet2", model_dict=md)
    blob = torch.load(got["checkpoint_path"], weights_only=True)
    assert set(blob["state_dict"]) == set(vm.state_dict()) and blob["epoch"] == 3 and blob["global_step"] == got["global_step"]
    torch.manual_seed(cfg.seed)
    init = VadModel("PyanNet2", md).state_dict()                                  # torch's own initialisation under the run's seed
    learning = [k for k in blob["state_dict"] if k.startswith(("model.lstm.", "model.linear.", "model.classifier."))]
    assert len(learning) == 2 * 2 * 4 + 4
    for k in learning:                                                            # every LSTM and head tensor moved
        assert not torch.equal(blob["state_dict"][k], init[k]), k
    again = entry.main(config(0.0, "again"))                                      # through main: the same run, the same numbers
    assert again["train_loss"] == got["train_loss"] and again["val_loss"] == got["val_loss"] and again["global_step"] == got["global_step"]
    assert set(again) == set(got) == {"train_loss", "val_loss", "val_metrics", "checkpoint_path", "global_step"}
    dropped = train_vad(**config(0.5, "dropped"))
    assert np.isfinite(dropped["train_loss"]).all() and dropped["train_loss"] != got["train_loss"]
    assert dropped["global_step"] == got["global_step"]
