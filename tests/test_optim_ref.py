"""The float64 mode of tests/optim_ref.py against torch float64 on the CPU (clip_grad_norm_ + Adam(weight_decay=), clip_grad_norm_ + AdamW,
a table of learning rates), and the schedule builders of scripts.lr_schedule_table against torch.optim.lr_scheduler.  What ties the f32
restatement the device is compared with (the same code path, other dtype) to the optimizers the reference trains with."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R

SIZES = (5000, 129, 37)          # three tensors of unequal size: more than one chunk, a ragged one, a tiny one
TABLE = (1e-3, 3e-3, 2e-3, 5e-4)


def _problem(seed=0):
    rng = np.random.default_rng(seed)
    w = [rng.standard_normal(n) * 0.3 for n in SIZES]
    grads = [[rng.standard_normal(n) * (1.0 + s) for n in SIZES] for s in range(10)]
    return w, grads


@pytest.mark.parametrize("decoupled", [False, True])
def test_float64_restatement_equals_torch_clip_plus_adam(decoupled):
    w0, grads = _problem()
    cfg = R.default_cfg(max_norm=1.5, weight_decay=1e-2, decoupled=decoupled)
    params = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in w0]
    make = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = make(params, lr=TABLE[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    fams, o = [R.family(w, f64=True) for w in w0], {"t": 0, "skipped": 0}
    clipped = 0
    for s in range(10):
        frames = 7 + s                                                           # the device divides the accumulated sum by the frame count
        for p, g in zip(params, grads[s]):
            p.grad = torch.tensor(g, dtype=torch.float64)
        for group in opt.param_groups:
            group["lr"] = TABLE[min(s, len(TABLE) - 1)]
        total = torch.nn.utils.clip_grad_norm_(params, 1.5)
        opt.step()
        fams, o, rec = R.step([(f, g * frames, frames) for f, g in zip(fams, grads[s])], o, cfg, TABLE, f64=True)
        clipped += rec["coef"] < 1.0
        assert abs(float(total) - rec["norm"]) <= 1e-12 * float(total) and rec["lr"] == TABLE[min(s, 3)] and rec["mask"] == 7
        for p, f in zip(params, fams):
            st = opt.state[p]
            for got, want in ((f["w"], p.detach().numpy()), (f["m"], st["exp_avg"].numpy()), (f["v"], st["exp_avg_sq"].numpy())):
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (s, decoupled)
    assert clipped == 10 and o == {"t": 10, "skipped": 0}


def test_f32_restatement_follows_the_float64_one_and_the_documented_norm_order():
    w0, grads = _problem(1)
    cfg = R.default_cfg(max_norm=1.5, weight_decay=1e-2)
    f32 = [R.family(w) for w in w0]
    f64 = [R.family(np.asarray(w, np.float32)) for w in w0]
    f64 = [R.family(f["w"], f64=True) for f in f64]
    o32 = o64 = {"t": 0, "skipped": 0}
    for s in range(3):
        acc = [np.asarray(g, np.float32) for g in grads[s]]
        f32, o32, r32 = R.step([(f, a, 1) for f, a in zip(f32, acc)], o32, cfg, TABLE)
        f64, o64, r64 = R.step([(f, a, 1) for f, a in zip(f64, acc)], o64, cfg, TABLE, f64=True)
        assert r32["norm"].dtype == np.float32 and abs(float(r32["norm"]) - r64["norm"]) <= 2.0 ** -23 * r64["norm"]
        for a, b in zip(f32, f64):
            assert a["w"].dtype == np.float32 and np.abs(a["w"] - b["w"]).max() <= 1e-5
    g = np.asarray(grads[0][0], np.float32)
    parts = R.chunk_partials(g)
    assert len(parts) == 2 and abs(sum(parts) - float(np.sum(g.astype(np.float64) ** 2))) <= 1e-12 * sum(parts)
    # absent and idle families add nothing; a step without a participant changes nothing
    fams, o, rec = R.step([None, (f32[1], np.zeros(129, np.float32), 0), None], {"t": 4, "skipped": 1}, cfg, TABLE)
    assert rec is None and o == {"t": 4, "skipped": 1} and fams[1]["t"] == f32[1]["t"] and np.array_equal(fams[1]["w"], f32[1]["w"])
    # a non-finite gradient: skipped, nothing but the counts move
    bad = np.asarray(grads[0][2], np.float32).copy()
    bad[3] = np.nan
    fams, o, rec = R.step([None, None, (f32[2], bad, 5)], {"t": 4, "skipped": 1}, R.default_cfg(skip_nonfinite=True), TABLE)
    assert rec["skipped"] and rec["coef"] == 0 and o == {"t": 4, "skipped": 2} and np.array_equal(fams[2]["m"], f32[2]["m"]) and rec["mask"] == 4


def _torch_lrs(make, steps=20, base=1e-3):
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=base)
    sched = make(opt)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return np.asarray(out, np.float64)


@pytest.mark.parametrize("schedule,make", [
    ({"name": "constant"}, lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda t: 1.0)),
    ({"name": "warmup", "warmup_steps": 6}, lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda t: min(1.0, (t + 1) / 6))),
    ({"name": "linear", "warmup_steps": 4}, lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda t: (t + 1) / 4 if t < 4 else 1.0 - (t - 4) / 16)),
    ({"name": "cosine"}, lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)),
    ({"name": "cosine", "eta_min": 1e-5}, lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20, eta_min=1e-5)),
    ({"name": "step", "step_size": 7, "gamma": 0.5}, lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=7, gamma=0.5)),
])
def test_schedule_tables_equal_torch_lr_schedulers_to_f32_rounding(schedule, make):
    from uvad_amd.scripts import lr_schedule_table
    got = lr_schedule_table(schedule, 1e-3, 20)
    want = _torch_lrs(make)
    assert got.shape == (20,) and (got.astype(np.float32) > 0).all()
    assert (np.abs(got.astype(np.float32).astype(np.float64) - want) <= 2.0 ** -23 * want).all()      # one f32 rounding of each entry


def test_schedule_builder_refuses_what_the_device_would():
    from uvad_amd.scripts import lr_schedule_table
    with pytest.raises(ValueError):
        lr_schedule_table({"name": "exponential"}, 1e-3, 5)
    with pytest.raises(ValueError):
        lr_schedule_table({"name": "warmup"}, 1e-3, 5)
    with pytest.raises(ValueError):
        lr_schedule_table({"name": "linear"}, 0.0, 5)
    assert lr_schedule_table(None, 2e-3, 3).tolist() == [2e-3] * 3
