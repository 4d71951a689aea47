"""Measure what dropout between the trainable LSTM layers costs (uvad_lstm_train_set_dropout): one training step of the top TWO LSTM layers
and the head (forward + uvad_head_train_grad + backward + both applies, as one graph replay) at 256 x 1000 frames, hidden 128
bidirectional, head 128 / 2, with p = 0 and with p = 0.5, on one GPU in one run: HIP events around blocks of replays, the two graphs
alternated block by block, median and spread over the blocks.  lt_dropout_kernel alone is timed the same way through uvad_dropout_apply,
in place over [256000][256] buffers taken in rotation (four of them, 1 GB together, so that no call finds its buffer in a cache), and its
bytes per second set beside the float4 copy of profiles/cuts.json.  Writes profiles/lstm_dropout.json.
Usage: python tools/run_lstm_dropout.py [--blocks 9] [--reps 10] [--out profiles/lstm_dropout.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBS = 6.29        # float4 copy on this GPU: profiles/cuts.json


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_dropout.json"))
    a = ap.parse_args()
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    B, T, F, layers = 256, 1000, 64, 2
    m = uvad_amd.PyanNet2(encoding_dim=F)                                 # 4 x 128 bidirectional, head 128 / 2: the top two layers and the head learn
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    g = torch.Generator().manual_seed(1)
    feats = (torch.randn(B, T, F, generator=g) * 2.0 - 3.0).to(dev)
    x_in = rt.lstm_train_input(feats, layers=layers).clone()              # the frozen two layers' output, cached
    y = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8).to(dev)

    graphs, handles = {}, {}
    for name, p in (("step_p0", 0.0), ("step_p05", 0.5)):
        hh, hl = rt.head_train_open(), rt.lstm_train_open(layers=layers, dropout=p, seed=0x5EED)

        def step(hh=hh, hl=hl):
            o = rt.lstm_train_forward(hl, x_in)
            _, gx = rt.head_train_grad(hh, o, y, want_grad_x=True)
            rt.lstm_train_backward(hl, x_in, gx)
            rt.head_train_apply(hh), rt.lstm_train_apply(hl)
        step()                                                            # sizes the workspaces
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            step()
        handles[name] = hl

    bufs = [torch.randn(B * T, 256, generator=torch.Generator(device=dev).manual_seed(k), device=dev) for k in range(4)]
    turn = [0]

    def drop_alone():
        turn[0] += 1
        b = bufs[turn[0] % 4]
        rt.dropout_apply(b, 2, turn[0], 0.5, 0x5EED, out=b)
    cands = {"step_p0": graphs["step_p0"].replay, "step_p05": graphs["step_p05"].replay, "lt_dropout_kernel": drop_alone}
    for fn in cands.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    draws0 = {k: rt.lstm_train_draws(h) for k, h in handles.items()}
    times = {k: [] for k in cands}
    for _ in range(a.blocks):                                             # alternated blocks: drift and clock state hit every candidate alike
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps)
    draws = {k: rt.lstm_train_draws(h) - draws0[k] for k, h in handles.items()}
    out = {"shape": {"B": B, "T": T, "Din": 256, "hidden": 128, "directions": 2, "trainable_layers": layers, "lin_hidden": 128, "lin_layers": 2,
                     "segment": "default (2048)"},
           "method": f"HIP events around blocks of {a.reps} calls, {a.blocks} blocks per candidate, candidates alternated block by block in one process; "
                     "each step is one graph replay; lt_dropout_kernel alone is uvad_dropout_apply in place over four [256000][256] buffers in rotation",
           "device": torch.cuda.get_device_name(0), "masks_drawn_while_timed": draws}
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()), "blocks_ms": [round(float(t), 4) for t in v]}
    p0, p5, dk = out["step_p0"], out["step_p05"], out["lt_dropout_kernel"]
    out["dropout_cost_ms"] = p5["ms_median"] - p0["ms_median"]
    out["dropout_cost_fraction_of_step"] = out["dropout_cost_ms"] / p0["ms_median"]
    out["ranges_resolve"] = bool(p5["ms_min"] > p0["ms_max"] or p5["ms_max"] < p0["ms_min"])
    nbytes = 2 * 4 * B * T * 256                                          # one 16-byte load and one 16-byte store per four columns
    out["lt_dropout_kernel"]["bytes_per_call"] = nbytes
    out["lt_dropout_kernel"]["tb_per_s"] = nbytes / (dk["ms_median"] * 1e-3) / 1e12
    out["lt_dropout_kernel"]["fraction_of_float4_copy"] = out["lt_dropout_kernel"]["tb_per_s"] / COPY_TBS
    out["lt_dropout_kernel"]["launches_per_step"] = 2 * (layers - 1)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"step_p0_ms": p0["ms_median"], "step_p05_ms": p5["ms_median"], "dropout_cost_ms": out["dropout_cost_ms"],
                      "fraction": out["dropout_cost_fraction_of_step"], "ranges_resolve": out["ranges_resolve"],
                      "kernel_ms": dk["ms_median"], "kernel_tb_per_s": out["lt_dropout_kernel"]["tb_per_s"], "masks_drawn": draws}))


if __name__ == "__main__":
    main()
