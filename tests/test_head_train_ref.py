"""The restatement of head fine-tuning (tests/head_train_ref.py) pinned to torch on the CPU: the float64 backward pass to torch.autograd on the
reference's own head expression (F.leaky_relu(linear(x)), F.binary_cross_entropy, frame weights and a length mask included); the f32 dz to
autograd through sigmoid + BCE over z in [-120, 120]; the f32 Adam step with running bias corrections to torch.optim.Adam over 100 steps."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_train_ref as R


def _params(D0, H, L, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    return {k: (rng.standard_normal(shape) * scale).astype(np.float32) for k, shape in R.keys(D0, H, L)}


@pytest.mark.parametrize("L,H,D0,slope", [(0, 0, 32, 0.01), (1, 32, 64, 0.01), (2, 64, 32, 0.01), (3, 32, 32, 0.5)])
def test_float64_backward_equals_autograd_on_the_reference_head(L, H, D0, slope):
    B, T = 3, 17
    rng = np.random.default_rng(10 + L)
    params = _params(D0, H, L, L)
    x = rng.standard_normal((B, T, D0)).astype(np.float32)
    y = rng.integers(0, 2, (B, T)).astype(np.uint8)
    w = rng.uniform(0.25, 2.0, (B, T)).astype(np.float32)
    lens = [T, 0, 9]
    x[1] = np.nan                                                 # past the lengths: never read
    x[2, 9:] = np.nan
    got = R.loss_and_grads(params, x, L, slope, y=y, w=w, lens=lens)
    valid = torch.from_numpy(R.valid_mask(B, T, lens))
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    xt = torch.tensor(np.nan_to_num(x), dtype=torch.float64, requires_grad=True)
    out = xt
    for l in range(L):
        out = F.leaky_relu(F.linear(out, tp[f"linear.{l}.weight"], tp[f"linear.{l}.bias"]), slope)
    p = torch.sigmoid(F.linear(out, tp["classifier.weight"], tp["classifier.bias"])).squeeze(-1)
    loss = F.binary_cross_entropy(p[valid], torch.from_numpy(y.astype(np.float64))[valid], weight=torch.from_numpy(w.astype(np.float64))[valid],
                                  reduction="sum")
    loss.backward()
    assert got["frames"] == int(valid.sum()) == T + 9
    assert abs(got["loss"] - loss.item()) <= 1e-12 * abs(loss.item())
    for k, g in got["grads"].items():
        want = tp[k].grad.numpy()
        assert np.abs(g.reshape(want.shape) - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), k
    gx = xt.grad.numpy()
    assert np.abs(got["grad_x"] - gx).max() <= 1e-12 * max(1.0, np.abs(gx).max())
    assert not got["grad_x"][1].any() and not got["grad_x"][2, 9:].any() and gx[0].any()
    # a caller's dz in place of the loss: the same backward pass
    again = R.loss_and_grads(params, x, L, slope, lens=lens, dz=got["dz"])
    assert again["loss"] == 0.0 and all(np.array_equal(again["grads"][k], got["grads"][k]) for k in got["grads"])


@pytest.mark.parametrize("label", [0, 1])
def test_f32_dz_equals_autograd_through_sigmoid_and_bce(label):
    """dz = w ((p - y) (q / max(q, 1e-12))) against autograd's ((p - y) / max(q, 1e-12) w) (1 - p) p on the same f32 p.  Both are the
    exact w (p - y) q / max(q, 1e-12) behind at most 4 (autograd) and 3 (here) f32 roundings: they differ by at most 8 x 2^-24 relative
    (measured: 3.2 x 2^-24), and both are exactly 0 where p rounds to 0 or 1."""
    z = torch.cat([torch.linspace(-120, 120, 9601), torch.tensor([-104.0, -103.9, -88.0, -87.3, -17.0, -16.6, 16.6, 17.0, 88.0])]).float()
    for wv in (1.0, 0.37):
        zz = z.clone().requires_grad_(True)
        p = torch.sigmoid(zz)
        w = torch.full_like(p, wv)
        F.binary_cross_entropy(p, torch.full_like(p, float(label)), weight=w, reduction="sum").backward()
        want = zz.grad.numpy()
        got = R.dz_f32(p.detach().numpy(), np.full(len(z), label), w.numpy())
        pn = p.detach().numpy()
        sat = (pn == 0) | (pn == 1)
        assert not got[sat].any() and not want[sat].any() and sat.sum() > 100            # exactly 0 where p rounds to 0 or 1
        assert (want[np.abs(z.numpy()) > 110] == 0).all() and (want != 0).sum() > 1000
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        normal = np.abs(want) >= 2.0 ** -100
        print("dz vs autograd, worst relative error in units of 2^-24:", float((err[normal] / np.abs(want[normal])).max() / 2.0 ** -24))
        # below the normal range (products of a subnormal p) either chain may underflow first: an absolute 2^-126 there
        assert (err <= 8 * 2.0 ** -24 * np.abs(want.astype(np.float64)) + 2.0 ** -126).all()
        f64 = R.dz_f64(pn, np.full(len(z), label), w.numpy())
        assert (np.abs(got - f64) <= 4 * 2.0 ** -24 * np.abs(f64) + 2.0 ** -126).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_f32_adam_with_running_corrections_tracks_torch_adam(seed):
    """100 steps of torch.optim.Adam (f32 tensors; bias corrections from beta ** step in f64, lerp_ with a fused multiply-add) beside
    the restatement (bias corrections advanced in f32 as c beta + (1 - beta), no fused operations) on weights of magnitude 0.5 .. 2, where an ulp is
    a meaningful unit.  Measured over seeds 0 .. 5: at most 2 ulp in the weights; 2 x that is asserted.  (With the running
    PRODUCT beta^t in f32 in place of the complement it was 10 ulp: 1 - (f32 nearest 0.999)^t is 1.3e-5 off.)  The moments are compared relative to their largest element (measured 1.5e-7 and 2.1e-7)."""
    rng = np.random.default_rng(seed)
    P = 4096
    w0 = (rng.uniform(0.5, 2.0, P) * rng.choice([-1, 1], P)).astype(np.float32)
    wt = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([wt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    w, st, worst = w0.copy(), R.adam_init(P), 0
    for i in range(100):
        frames = 37 + i
        acc = (rng.standard_normal(P) * frames).astype(np.float32)
        wt.grad = torch.from_numpy((acc / np.float32(frames)).astype(np.float32))
        opt.step()
        w, st = R.adam_step(w, acc, frames, st)
        worst = max(worst, int(np.abs(w.view(np.int32).astype(np.int64) - wt.detach().numpy().view(np.int32).astype(np.int64)).max()))
    print("Adam restatement vs torch.optim.Adam after 100 steps: worst distance", worst, "ulp")
    assert worst <= 4
    sd = opt.state_dict()["state"][0]
    assert np.abs(st["m"] - sd["exp_avg"].numpy()).max() <= 1e-6 * np.abs(st["m"]).max()
    assert np.abs(st["v"] - sd["exp_avg_sq"].numpy()).max() <= 1e-6 * np.abs(st["v"]).max()
    assert st["t"] == 100 and abs(float(st["bc1"]) - (1 - 0.9 ** 100)) <= 1e-6 and abs(float(st["bc2"]) - (1 - 0.999 ** 100)) <= 1e-6 * (1 - 0.999 ** 100)
    same_w, same = R.adam_step(w, np.ones(P, np.float32), 0, st)   # no frames: no step
    assert same is st and same_w is w


def test_pack_and_unpack_follow_state_dict_order():
    ks = [k for k, _ in R.keys(64, 32, 2)]
    assert ks == ["linear.0.weight", "linear.0.bias", "linear.1.weight", "linear.1.bias", "classifier.weight", "classifier.bias"]
    lin = torch.nn.ModuleList([torch.nn.Linear(64, 32), torch.nn.Linear(32, 32)])
    sd = {f"linear.{k}": v for k, v in lin.state_dict().items()}
    assert list(sd) == ks[:4]
    params = _params(64, 32, 2, 5)
    flat = R.pack(params, 64, 32, 2)
    assert flat.size == 64 * 32 + 32 + 32 * 32 + 32 + 32 + 1
    back = R.unpack(flat, 64, 32, 2)
    assert all(np.array_equal(back[k], params[k]) for k in ks)
    assert [k for k, _ in R.keys(96, 0, 0)] == ["classifier.weight", "classifier.bias"] and R.keys(96, 0, 0)[0][1] == (1, 96)


def test_exactness_margin_flags_what_f32_cannot_sum_exactly():
    rng = np.random.default_rng(3)
    params = {k: rng.integers(-1, 2, shape).astype(np.float32) for k, shape in R.keys(32, 32, 1)}
    x = rng.integers(-2, 3, (2, 5, 32)).astype(np.float32)
    dz = rng.integers(-2, 3, (2, 5)).astype(np.float32)
    big, grid = R.exactness_margin(params, x, 1, 0.5, dz)
    assert big < 2 ** 20 and grid >= 2.0 ** -4
    params["linear.0.weight"][0, 0] = 0.3
    assert R.exactness_margin(params, x, 1, 0.5, dz)[1] < 2.0 ** -4
    params["linear.0.weight"][0, 0] = 2.0 ** 21
    x[0, 0, 0] = 1
    assert R.exactness_margin(params, x, 1, 0.5, dz)[0] >= 2 ** 20
