"""Training at the size of the model the reference ships (4 bidirectional layers of 128 units on 80 features, 5 s windows of 500 frames, the
default gradient segment), which the neighbouring files reach only at toy sizes:

  1  recurrence and contractions   shape R (80 -> 4 x 128 x 2, B 6, T 500, lengths 500 / 317 / 1 / 500 / 64 / 0, N = 3000: two default segments,
                                   the second of 29 full k-chunks and a ragged one of 24) and R2 (80 -> 2 x 64 x 2, B 7, lengths around T - 1 and
                                   the prefetch depth): exact structure as test_gpu_lstm_train.py holds it, rows alone, and the 4 x torch-f32 bound
  2  batch-tile tails              B in {2, 3, 6, 7}: last tiles of 2 and 3 rows on a workspace of 0xFF bytes, every row against the row alone
  3  the joint step                LSTM families of 256, 257 and 342 reduction chunks: opt_fold_kernel's second pass through LDS, bit for bit
                                   against optim_ref.step, and the read -> write -> continue round trip at 342
  4  the whole step                PyanNet2 of two layers at T 500, five Adam steps against the float64 torch loop

The float64 restatements and the torch comparators are computed once per process and shared (_reference, _loss_loops).  What the GPU tests
divide by is conditioned in a test that needs no GPU: torch's own f32 error at most 1e-5 of every tensor's float64 max-abs on every seed used,
no float64 gradient tensor identically zero, and the f32 loss loop within 1e-4 of the first loss of the float64 loop."""
import functools

import numpy as np
import pytest
import torch

import head_train_ref as HR
import lstm_train_ref as R
import optim_ref as OR
import test_gpu_lstm_train as T0
import test_gpu_optim as T3
from test_gpu_lstm_train import Trainer, _lens_d, _poisoned, _pooled_ratios, _runtime

gpu = pytest.mark.gpu
PAD = T0.PAD
F32 = np.float32
_bits = T0._bits

# name: ((Din, H, dirs, layers, first_layer), B, T, lengths)
SHAPES = {"R": ((80, 128, 2, 4, 0), 6, 500, (500, 317, 1, 500, 64, 0)),
          "R2": ((80, 64, 2, 2, 0), 7, 500, (500, 499, 3, 250, 500, 4, 5))}
SEEDS = (0, 1, 2)
TORCH_F32_CAP = 1e-5      # torch f32 against float64 measures 0.8e-6 .. 1.3e-6 at T 500; a chaotic recurrence would be orders above the cap


# ------------------------------------------------------------------------------------------------ the shared references
@functools.lru_cache(maxsize=None)
def _reference(name, seed):
    """The seeded problem of SHAPES[name], its float64 restatement and torch f32 autograd on the CPU: computed once, left unchanged."""
    shape, B, T, lens = SHAPES[name]
    Din, H, dirs, layers, first = shape
    params, x, dy = R.seeded(100 + seed, *shape, B, T, scale=2.0)
    truth = R.forward_backward(params, x, dy, H, dirs, layers, first, list(lens))
    truth = {"y": truth["y"], "grads": truth["grads"], "grad_in": truth["grad_in"]}      # the kept activations are not needed again
    cpu = R.torch_forward_backward(params, x, dy, H, dirs, layers, first, list(lens), dtype=torch.float32)
    return {"params": params, "x": x, "dy": dy, "truth": truth, "cpu": cpu}


def _tensors(d):
    return [("y", d["y"]), ("grad_in", d["grad_in"])] + list(d["grads"].items())


def _seeded_sd(Din, H, layers, seed, scale):
    """The state dict test_gpu_lstm_train._runtime loads for these arguments, without a runtime."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet2(lstm={"hidden_size": H, "num_layers": layers, "bidirectional": True}, linear={"hidden_size": 32, "num_layers": 1},
                          encoding_dim=Din)
    m.build()
    seed_weights(m, seed, scale)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


STEP = dict(Din=80, H=64, layers=2, B=5, T=500, lens=(500, 317, 64, 500, 9), lr=3e-3, steps=5)


@functools.lru_cache(maxsize=None)
def _loss_loops(seed):
    """Part 4's problem for one seed and the losses of five Adam steps of the torch loop on the CPU in float64 and in f32."""
    c = STEP
    sd = _seeded_sd(c["Din"], c["H"], c["layers"], 40 + seed, 2.0)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((c["B"], c["T"], c["Din"])).astype(np.float32)
    y = (x[..., :8].sum(-1) > 0).astype(np.uint8)
    v = torch.from_numpy(HR.valid_mask(c["B"], c["T"], list(c["lens"])))
    loops = {}
    for dtype in (torch.float64, torch.float32):
        prm, fwd = T0._torch_model(sd, c["Din"], c["H"], dtype, layers=c["layers"])
        opt = torch.optim.Adam(prm, lr=c["lr"])
        xt, yt, losses = torch.tensor(x, dtype=dtype), torch.from_numpy(y).to(dtype), []
        for _ in range(c["steps"]):
            opt.zero_grad()
            loss = torch.nn.functional.binary_cross_entropy(fwd(xt, list(c["lens"]))[v], yt[v])
            losses.append(loss.item())
            loss.backward()
            opt.step()
        loops[dtype] = np.array(losses)
    return {"sd": sd, "x": x, "y": y, "f64": loops[torch.float64], "f32": loops[torch.float32]}


def _torch_loop_deviation():
    """(rms deviation of torch's f32 losses from the float64 loop pooled over SEEDS, the smallest first loss)."""
    dev2 = [float(((_loss_loops(s)["f32"] - _loss_loops(s)["f64"]) ** 2).mean()) for s in SEEDS]
    return float(np.sqrt(np.mean(dev2))), min(float(_loss_loops(s)["f64"][0]) for s in SEEDS)


# ------------------------------------------------------------------------------------------------ the conditions on the inputs (no GPU)
def test_torch_f32_is_accurate_and_every_gradient_is_live_on_the_inputs_the_gpu_tests_use():
    """The ratios of parts 1 and 4 mean something only while their denominators do.  Per shape, seed and tensor: torch f32's max error over
    the float64 tensor's max-abs at most 1e-5 (measured 0.8e-6 .. 1.3e-6; a seed that fails is replaced, the cap stays), the float64 max-abs
    not zero.  Part 4: the f32 loop's pooled rms deviation from the float64 loop not zero and below 1e-4 of the first loss, the float64 loss
    falling on every seed."""
    for name in SHAPES:
        for seed in SEEDS:
            ref = _reference(name, seed)
            worst = (0.0, None)
            cpu = dict(_tensors(ref["cpu"]))
            for k, t in _tensors(ref["truth"]):
                c, scale = cpu[k], float(np.abs(t).max())
                assert scale > 0.0, (name, seed, k)
                e = float(np.abs(np.asarray(c, np.float64).reshape(t.shape) - t).max()) / scale
                worst = max(worst, (e, k))
                assert e <= TORCH_F32_CAP, (name, seed, k, e)
            print(f"{name} seed {seed}: torch f32 worst error {worst[0]:.2e} ({worst[1]}) over {len(_tensors(ref['truth']))} tensors")
    t, first = _torch_loop_deviation()
    for s in SEEDS:
        lo = _loss_loops(s)
        print(f"whole step seed {s}: float64 loss {lo['f64'][0]:.6f} -> {lo['f64'][-1]:.6f}, torch f32 deviation "
              f"{float(np.sqrt(((lo['f32'] - lo['f64']) ** 2).mean())):.3e}")
        assert lo["f64"][-1] < lo["f64"][0], s
    print(f"whole step: torch f32 pooled rms deviation {t:.3e}, {t / first:.2e} of the first loss {first:.6f}")
    assert 0.0 < t < 1e-4 * first


# ------------------------------------------------------------------------------------------------ 1. window length, reference depth
def _device_case(name, seed, runs=1):
    """Forward and backward of _reference(name, seed) from reset, `runs` times, on NaN past the lengths
    -> (runtime, trainer, inputs on the device, [(y, grad_in, gradient, state bytes)] per run)."""
    shape, B, T, lens = SHAPES[name]
    ref = _reference(name, seed)
    rt, _, _ = _runtime(*shape[:4], ref["params"])
    tr = Trainer(rt, segment=0)                                                   # the default segment: N = B T spans two of them
    valid = HR.valid_mask(B, T, list(lens))
    xd, dd = _poisoned(ref["x"], ref["dy"], valid)
    out = []
    for _ in range(runs):
        tr.reset()
        y = tr.forward(xd, _lens_d(list(lens)))
        gin = tr.backward(xd, dd, _lens_d(list(lens)))
        torch.cuda.synchronize()
        out.append((y.cpu().numpy(), gin.cpu().numpy(), tr.grad(), bytes(tr.sbuf.cpu().numpy())))
    return rt, tr, (xd, dd, valid), out


@gpu
def test_window_length_at_reference_depth_keeps_the_exact_structure_and_rows_equal_the_rows_alone():
    """Shape R, seed 0.  Tile 0 mixes the lengths 500 / 317 / 1 / 500 (a workgroup of 500 steps holding a one-frame row's zero state for 499 of
    them in the reverse direction), tile 1 holds two rows, one empty.  Row-local, as in test_a_row_inside_a_ragged_batch_...: y and grad_in."""
    shape, B, T, lens = SHAPES["R"]
    rt, tr, (xd, dd, valid), runs = _device_case("R", 0, runs=2)
    (y, gin, g, sa), (y2, gin2, g2, sb) = runs
    assert y.tobytes() == y2.tobytes() and gin.tobytes() == gin2.tobytes() and sa == sb      # two runs from reset: the same bytes
    assert not _bits(y[~valid]).any() and not _bits(gin[~valid]).any()            # +0 past the lengths, NaN there in x and dy
    assert np.isfinite(y).all() and np.isfinite(gin).all() and np.isfinite(g).all()
    assert tr.read(tr.L.HEAD_TRAIN_SCALARS)["frames"] == int(valid.sum()) == sum(lens)
    got = R.unpack(g, *shape)
    assert len(got) == 32
    for k in got:
        assert _bits(got[k]).any(), k
        if "bias_hh" in k:
            assert np.array_equal(_bits(got[k]), _bits(got[k.replace("bias_hh", "bias_ih")])), k
    ref = _reference("R", 0)["truth"]                                             # the sanity net of the structure tier; the bound is the next test's
    for name, a, b in [("y", y, ref["y"]), ("grad_in", gin, ref["grad_in"])] + [(k, got[k], ref["grads"][k]) for k in got]:
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), name
    yd, gd = torch.from_numpy(y).to(xd.device), torch.from_numpy(gin).to(xd.device)
    for b in (1, 4):                                                              # lengths 317 and 64, alone as B = 1, T = 500
        one = Trainer(rt, segment=0)
        x1, d1 = xd[b:b + 1].contiguous(), dd[b:b + 1].contiguous()
        y1 = one.forward(x1, _lens_d([lens[b]]))
        g1 = one.backward(x1, d1, _lens_d([lens[b]]))
        assert torch.equal(y1[0], yd[b]) and torch.equal(g1[0], gd[b]), b
        assert not _bits(y1[0, lens[b]:].cpu().numpy()).any() and one.canaries_intact()
    assert tr.canaries_intact()
    rt.close()


@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_output_and_gradients_at_window_length_within_four_times_torch_f32_autograd(name):
    """test_output_and_gradients_within_four_times_torch_f32_autograd's figures and bound (at most 4 x torch f32, rms and max
    of the error against float64 over the float64 max-abs, pooled over three seeds) for y, grad_in and every gradient tensor at T 500."""
    shape, B, T, lens = SHAPES[name]
    cases, refs = [], []
    for seed in SEEDS:
        ref = _reference(name, seed)
        rt, tr, _, [(y, gin, g, _)] = _device_case(name, seed)
        assert tr.canaries_intact()
        cases.append((ref["params"], ref["x"], ref["dy"], list(lens), dict(R.unpack(g, *shape), y=y, grad_in=gin), shape))
        refs.append((ref["truth"], ref["cpu"]))
        rt.close()
    worst = 0.0
    pooled = _pooled_ratios(cases, shape[3], shape[4], refs=refs)
    assert len(pooled) == 2 + 8 * shape[3]
    for k, f in pooled.items():
        ratios = (f["kernel"][0] / f["torch"][0], f["kernel"][1] / f["torch"][1])
        worst = max(worst, *ratios)
        print(f"{name} {k}: kernel rms {f['kernel'][0]:.2e} max {f['kernel'][1]:.2e} | torch f32 rms {f['torch'][0]:.2e} max {f['torch'][1]:.2e} | "
              f"ratios {ratios[0]:.2f} {ratios[1]:.2f}")
    print(f"{name}: worst ratio {worst:.2f}")
    assert worst <= 4.0


# ------------------------------------------------------------------------------------------------ 2. batch-tile tails
@functools.lru_cache(maxsize=None)
def _tail_problem():
    shape = (60, 64, 2, 1, 0)
    params, x, dy = R.seeded(77, *shape, 7, 9, scale=2.0)
    return shape, params, x, dy, _runtime(*shape[:4], params)[0]


def _on_a_poisoned_workspace(tr, x, dy=None):
    """forward (and backward) on a workspace whose every byte is 0xFF: one forward of the same shape first, so that the workspace exists."""
    tr.forward(x)
    (w,) = tr.ws.values()
    tr.reset()
    w[PAD:w.numel() - PAD] = 0xFF
    y = tr.forward(x)
    return y, (tr.backward(x, dy) if dy is not None else None)


@gpu
@pytest.mark.parametrize("B", [2, 3, 6, 7])
def test_every_row_of_a_batch_whose_last_tile_is_not_full_equals_the_row_alone(B):
    """B mod 4 in {2, 3}: the last 4-sequence tile holds lanes past the batch.  Every row's y and grad_in equal the row alone bit for bit, and
    so do the kept activations, seen through the gradients of a dy that is zero outside the row: the other rows' dpre are then zeros, which an
    f32 chain in frame order passes through unchanged.  A gradient partial is a sum of 32-frame chunk sums, so this holds bit for bit for a
    row that lies inside one chunk.  Row 3 (frames 27 .. 35) straddles a chunk boundary and its nine terms are associated differently from
    the row alone: at most 8 roundings of 2^-24 on either side, each relative to at most nine times the largest term; with no term above the
    tensor's largest entry that is 2 * 8 * 9 * 2^-24 = 8.6e-6 of the tensor's max-abs, a net a lane of another row or of 0xFF bytes tears."""
    shape, params, x, dy, rt = _tail_problem()
    T, H = 9, shape[1]
    xd, dd = T0._to(x[:B]), T0._to(dy[:B])
    tr = Trainer(rt, segment=0)
    y, gin = _on_a_poisoned_workspace(tr, xd, dd)
    assert torch.isfinite(y).all() and torch.isfinite(gin).all()
    for b in range(B):
        one = Trainer(rt, segment=0)
        y1, g1 = _on_a_poisoned_workspace(one, xd[b:b + 1].contiguous(), dd[b:b + 1].contiguous())
        assert torch.equal(y1[0], y[b]) and torch.equal(g1[0], gin[b]), b
        alone = R.unpack(one.grad(), *shape)
        only = torch.zeros_like(dd)
        only[b] = dd[b]
        _on_a_poisoned_workspace(tr, xd, only)
        inside = R.unpack(tr.grad(), *shape)
        one_chunk = b * T // 32 == (b * T + T - 1) // 32
        for k in alone:
            assert _bits(alone[k]).any(), k
            if one_chunk:
                assert np.array_equal(_bits(inside[k]), _bits(alone[k])), (b, k)
            else:
                assert np.abs(inside[k] - alone[k]).max() <= 144 * 2.0 ** -24 * np.abs(alone[k]).max(), (b, k)
        assert one.canaries_intact()
    assert tr.canaries_intact()


# ------------------------------------------------------------------------------------------------ 3. more than 256 chunks per family
# (layers, Din) -> (LSTM P, chunks): 256 with a ragged last chunk is one LDS pass with n == 256; 257 a second pass with n == 1 whose only
# partial is a ragged half chunk; 342 full chunks the reference model, a second pass with n == 86
BIG = {(3, 120): (1046528, 256), (3, 124): (1050624, 257), (4, 80): (1400832, 342)}


@gpu
@pytest.mark.parametrize("layers,Din", list(BIG))
def test_the_joint_step_over_a_family_of_256_and_more_chunks_equals_the_restatement(layers, Din):
    """H 128 bidirectional, head 32 / 1, B 2, T 5, lengths (5, 2), segment 32: three clipped, decayed steps equal optim_ref.step bit for bit
    (norm, coef, lr, mask, counts, w, m, v, bc1, bc2 of both families), max_norm at half the first step's norm.  At 342 chunks the states
    then move through read / write into a fresh context, whose third step lands on the bytes of the uninterrupted one."""
    P, chunks = BIG[(layers, Din)]
    shape = dict(Din=Din, H=128, layers=layers, B=2, T=5, lens=(5, 2))
    table = [1e-3, 2e-3, 5e-4]
    probe = T3.Chain("lstm", **shape)
    rt = probe.rt
    rt._lstm_train_configure(probe.hl)
    assert int(rt.lib.uvad_lstm_train_param_count(rt.ctx)) == P == probe.hl["P"]  # a change of layout must not move the case off its edge
    assert (P + OR.CHUNK - 1) // OR.CHUNK == chunks and (P % OR.CHUNK != 0) == (chunks != 342)
    probe.fb(0)                                                                   # the first step's norm, from the accumulators as read
    gs = [(s["g"] / F32(s["frames"])).astype(F32) for s in probe.snap()[:2]]
    first = F32(np.sqrt(OR.sum_squares(gs)))
    assert first > 0
    cfg = {"max_norm": 0.5 * float(first), "weight_decay": 1e-2}
    ch = T3.Chain("lstm", rt=rt, **shape)                                         # fresh states on the same context
    o = ch.optim_open(cfg, table, canaries=True)
    ref, ropt = T3._ref_of(ch.snap()), {"t": 0, "skipped": 0}
    other = None
    for k in range(3):
        if k == 2 and chunks == 342:
            saved, rec = ch.reads(), rt.optim_read(o)
            other = T3.Chain("lstm", **shape)                                     # a fresh context: reset from the initial weights, then written
            oo = other.optim_open(cfg, table, canaries=True)
            other.rt.head_train_write(other.hh, saved[0])
            other.rt.lstm_train_write(other.hl, saved[1])
            other.rt.optim_write(oo, rec)
            assert other.state_bytes() == ch.state_bytes() and bytes(oo["state"].cpu().numpy()) == bytes(o["state"].cpu().numpy())
        ref, ropt, rec = T3._checked_step(ch, o, ref, ropt, cfg, table, k)
        print(f"layers {layers} Din {Din} ({chunks} chunks) step {k}: norm {float(rec['norm']):.9g} coef {float(rec['coef']):.9g} "
              f"lr {float(rec['lr']):.9g}")
        if k == 0:
            assert rec["coef"] < 1.0 and _bits(rec["norm"]) == _bits(first)
    if other is not None:
        other.fb(2), other.optim(oo)
        assert other.state_bytes() == ch.state_bytes() and bytes(oo["state"].cpu().numpy()) == bytes(o["state"].cpu().numpy())
        assert other.canaries_intact()
        other.rt.close()
    assert ch.canaries_intact() and rt.optim_read(o)["step"] == 3
    rt.close()


# ------------------------------------------------------------------------------------------------ 4. the whole step at window length
@gpu
def test_five_steps_of_the_two_layer_chain_at_window_length_track_the_float64_torch_loop():
    """test_twenty_steps_of_the_full_chain_track_the_float64_torch_loop at T 500 with two layers (N = 2500: two default segments in the head's
    and the LSTM's weight-gradient kernels), the _apply path: the rms deviation of the five losses from the float64 torch loop, pooled over
    three seeds, at most 4 x the deviation of torch's own f32 loop; the loss ends below where it started."""
    c = STEP
    dev2 = []
    for seed in SEEDS:
        lo = _loss_loops(seed)
        rt, sd, _ = _runtime(c["Din"], c["H"], 2, c["layers"], seed=40 + seed, scale=2.0)
        assert all(torch.equal(sd[k], lo["sd"][k]) for k in sd)                   # the model the torch loops trained
        hh, hl = rt.head_train_open(lr=c["lr"]), rt.lstm_train_open(layers=c["layers"], lr=c["lr"])
        xd, yd, ld = T0._to(lo["x"]), T0._to(lo["y"]), _lens_d(list(c["lens"]))
        got = []
        for _ in range(c["steps"]):
            out = rt.lstm_train_forward(hl, xd, lengths=ld)
            _, gx = rt.head_train_grad(hh, out, yd, lengths=ld, want_grad_x=True)
            rt.lstm_train_backward(hl, xd, gx, lengths=ld)
            got.append(rt.head_train_batch_loss(hh).clone())
            rt.head_train_apply(hh)
            rt.lstm_train_apply(hl)
        torch.cuda.synchronize()
        got = np.array([float(l) for l in got])
        dev2.append(float(((got - lo["f64"]) ** 2).mean()))
        print(f"seed {seed}: loss {lo['f64'][0]:.6f} -> {lo['f64'][-1]:.6f} (float64), kernel {got[0]:.6f} -> {got[-1]:.6f}")
        assert got[-1] < got[0] and lo["f64"][-1] < lo["f64"][0]
        assert rt.lstm_train_read(hl)["step"] == c["steps"]
        rt.close()
    k, (t, _) = float(np.sqrt(np.mean(dev2))), _torch_loop_deviation()
    print(f"rms deviation of {c['steps']} losses from the float64 loop, three seeds: kernel {k:.3e}, torch f32 {t:.3e}, ratio {k / t:.2f}")
    assert k <= 4.0 * t
