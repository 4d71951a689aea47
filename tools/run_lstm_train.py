"""Measure one training step of the top LSTM layer and the head (uvad_lstm_train_forward + uvad_head_train_grad + uvad_lstm_train_backward +
both applies, as one graph replay) at 256 x 1000 frames, hidden 128 bidirectional, one trainable layer, head 128 / 2, beside the same step
in torch-ROCm autograd (nn.LSTM + the head) + torch.optim.Adam, on one GPU in one run: HIP events around blocks of calls, the candidates
alternated block by block, median and spread over the blocks.  The phases of the step (forward, head, backward, applies) are timed the
same way as eager calls.  Writes profiles/lstm_train.json; a "kernel_split" entry already in that file (medians per kernel from a
kernel-trace run of this tool with --blocks 1 --reps 3) is carried over.
Usage: python tools/run_lstm_train.py [--blocks 9] [--reps 10] [--out profiles/lstm_train.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_train.json"))
    a = ap.parse_args()
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    B, T, F, Hh, D0, H, L = 256, 1000, 64, 128, 256, 128, 2
    m = uvad_amd.PyanNet2(encoding_dim=F)                                 # 4 x 128 bidirectional, head 128 / 2: the top layer and the head learn
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    g = torch.Generator().manual_seed(1)
    feats = (torch.randn(B, T, F, generator=g) * 2.0 - 3.0).to(dev)
    x_in = rt.lstm_train_input(feats, layers=1).clone()                   # the frozen three layers' output, cached
    y = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8).to(dev)

    hh, hl = rt.head_train_open(), rt.lstm_train_open(layers=1)
    out_y = rt.lstm_train_forward(hl, x_in)                               # sizes the workspaces
    _, gx = rt.head_train_grad(hh, out_y, y, want_grad_x=True)
    rt.lstm_train_backward(hl, x_in, gx)
    rt.head_train_apply(hh), rt.lstm_train_apply(hl)
    torch.cuda.synchronize()

    def step():
        o = rt.lstm_train_forward(hl, x_in)
        _, gxx = rt.head_train_grad(hh, o, y, want_grad_x=True)
        rt.lstm_train_backward(hl, x_in, gxx)
        rt.head_train_apply(hh), rt.lstm_train_apply(hl)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()

    sd = m.state_dict()
    lstm = torch.nn.LSTM(D0, Hh, 1, batch_first=True, bidirectional=True)
    lin = [torch.nn.Linear(D0, H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)]
    with torch.no_grad():
        for name, prm in lstm.named_parameters():
            prm.copy_(sd["lstm." + name.replace("_l0", "_l3")])
        for i, mod in enumerate(lin):
            pre = f"linear.{i}" if i < 2 else "classifier"
            mod.weight.copy_(sd[pre + ".weight"]), mod.bias.copy_(sd[pre + ".bias"])
    lstm, lin = lstm.to(dev), [mod.to(dev) for mod in lin]
    opt = torch.optim.Adam(list(lstm.parameters()) + [p for mod in lin for p in mod.parameters()], lr=1e-3)
    yf = y.float()

    def torch_step():
        opt.zero_grad(set_to_none=True)
        o, _ = lstm(x_in)
        o = torch.nn.functional.leaky_relu(lin[1](torch.nn.functional.leaky_relu(lin[0](o))))
        torch.nn.functional.binary_cross_entropy(torch.sigmoid(lin[2](o)).squeeze(-1), yf).backward()
        opt.step()

    cands = {"lstm_train_graph": graph.replay, "torch_autograd_adam": torch_step,
             "phase_forward": lambda: rt.lstm_train_forward(hl, x_in),
             "phase_head_grad": lambda: rt.head_train_grad(hh, out_y, y, want_grad_x=True),
             "phase_backward": lambda: rt.lstm_train_backward(hl, x_in, gx),
             "phase_applies": lambda: (rt.head_train_apply(hh), rt.lstm_train_apply(hl))}
    for fn in cands.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
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
    out = {"shape": {"B": B, "T": T, "Din": D0, "hidden": Hh, "directions": 2, "trainable_layers": 1, "lin_hidden": H, "lin_layers": L,
                     "segment": "default (2048)"},
           "method": f"HIP events around blocks of {a.reps} calls, {a.blocks} blocks per candidate, candidates alternated block by block in one process; "
                     "the phases are eager calls of the runtime's wrappers (output allocation included), the step is one graph replay",
           "device": torch.cuda.get_device_name(0),
           "lstm_workspace_bytes": int(rt.lib.uvad_lstm_train_ws_bytes(rt.ctx, B, T)), "lstm_state_bytes": int(rt.lib.uvad_lstm_train_state_bytes(rt.ctx)),
           "lstm_param_count": int(rt.lib.uvad_lstm_train_param_count(rt.ctx))}
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()), "blocks_ms": [round(float(t), 4) for t in v]}
    out["ratio_to_torch"] = out["lstm_train_graph"]["ms_median"] / out["torch_autograd_adam"]["ms_median"]
    out["ranges_resolve"] = bool(out["lstm_train_graph"]["ms_min"] > out["torch_autograd_adam"]["ms_max"] or
                                 out["lstm_train_graph"]["ms_max"] < out["torch_autograd_adam"]["ms_min"])
    if os.path.exists(a.out):                                             # the per-kernel split comes from a separate kernel-trace run: keep it
        try:
            old = json.load(open(a.out))
            if "kernel_split" in old:
                out["kernel_split"] = old["kernel_split"]
        except ValueError:
            pass
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (out[k]["ms_median"] if isinstance(out[k], dict) and "ms_median" in out[k] else out[k])
                      for k in list(cands) + ["ratio_to_torch", "ranges_resolve", "lstm_workspace_bytes"]}))


if __name__ == "__main__":
    main()
