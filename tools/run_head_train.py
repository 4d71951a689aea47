"""Measure one head fine-tuning step (uvad_head_train_grad + uvad_head_train_apply as one graph replay) at 256 x 1000 frames, D0 = 256,
head 128 / 2, beside the same step in torch-ROCm autograd + torch.optim.Adam and beside one uvad_classify of the same batch, on one GPU
in one run: HIP events around blocks of replays, the three candidates alternated block by block, median and spread over the blocks.
Writes profiles/head_train.json.  Usage: python tools/run_head_train.py [--blocks 9] [--reps 10] [--out profiles/head_train.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train.json"))
    ap.add_argument("--accuracy", default="", help="a JSON file of measured accuracy ratios to carry into the output")
    a = ap.parse_args()
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    B, T, F, D0, H, L = 256, 1000, 64, 256, 128, 2
    m = uvad_amd.PyanNet2(encoding_dim=F)
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    g = torch.Generator().manual_seed(1)
    feats = (torch.randn(B, T, F, generator=g) * 2.0 - 3.0).to(dev)
    rt.classify(feats)
    x0 = rt.taps(lin=False)[0].clone()
    y = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8).to(dev)

    h = rt.head_train_open()
    rt.head_train_grad(h, x0, y)                                      # sizes the workspace
    rt.head_train_apply(h)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rt.head_train_grad(h, x0, y)
        rt.head_train_apply(h)

    lin = [torch.nn.Linear(D0, H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)]
    sd = m.state_dict()
    with torch.no_grad():
        for i, mod in enumerate(lin):
            pre = f"linear.{i}" if i < 2 else "classifier"
            mod.weight.copy_(sd[pre + ".weight"]), mod.bias.copy_(sd[pre + ".bias"])
    lin = [mod.to(dev) for mod in lin]
    opt = torch.optim.Adam([p for mod in lin for p in mod.parameters()], lr=1e-3)
    yf = y.float()

    def torch_step():
        opt.zero_grad(set_to_none=True)
        o = torch.nn.functional.leaky_relu(lin[1](torch.nn.functional.leaky_relu(lin[0](x0))))
        torch.nn.functional.binary_cross_entropy(torch.sigmoid(lin[2](o)).squeeze(-1), yf).backward()
        opt.step()

    cands = {"head_train_graph": graph.replay, "torch_autograd_adam": torch_step, "uvad_classify": lambda: rt.classify(feats)}
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(a.blocks):                                         # alternated blocks: drift and clock state hit every candidate alike
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps)
    N = B * T
    flop = 6.0 * N * (D0 * H + (L - 1) * H * H + H)
    out = {"shape": {"B": B, "T": T, "D0": D0, "lin_hidden": H, "lin_layers": L, "segment": "default (2048)"},
           "method": f"HIP events around blocks of {a.reps} calls, {a.blocks} blocks per candidate, candidates alternated block by block in one process",
           "device": torch.cuda.get_device_name(0), "flop_per_step": flop,
           "workspace_bytes": int(rt.lib.uvad_head_train_ws_bytes(rt.ctx, B, T)), "state_bytes": int(rt.lib.uvad_head_train_state_bytes(rt.ctx))}
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()), "blocks_ms": [round(float(t), 4) for t in v]}
    out["fraction_of_f32_matrix_peak_157TFLOPs"] = flop / (out["head_train_graph"]["ms_median"] * 1e-3) / 157.3e12
    if a.accuracy and os.path.exists(a.accuracy):
        out["accuracy_vs_float64"] = json.load(open(a.accuracy))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("head_train_graph", "torch_autograd_adam", "uvad_classify", "fraction_of_f32_matrix_peak_157TFLOPs", "workspace_bytes")}))


if __name__ == "__main__":
    main()
