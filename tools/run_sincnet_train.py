"""Measure one full PyanNet training step (uvad_sincnet_train_forward -> uvad_lstm_train_forward -> uvad_head_train_grad ->
uvad_lstm_train_backward -> uvad_sincnet_train_backward -> the three applies, as one graph replay) at 256 x 5 s of waveform, hidden 128
bidirectional, 4 layers, head 128 / 2, beside the same step in torch-ROCm autograd (the SincNet of tests/sincnet_train_ref.py, nn.LSTM, the
head) + torch.optim.Adam, on one GPU in one run: HIP events around blocks of calls, the candidates alternated block by block, median and
spread over the blocks.  The SincNet phases (forward, backward, apply) are timed the same way as eager calls; their sum over the step is the
front end's share.  Writes profiles/sincnet_train.json; a "kernel_split" entry already in that file (medians per kernel from a kernel-trace
run of this tool with --blocks 1 --reps 2) is carried over.
Usage: python tools/run_sincnet_train.py [--blocks 7] [--reps 3] [--batch 256] [--out profiles/sincnet_train.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sincnet_train.json"))
    a = ap.parse_args()
    import sincnet_train_ref as R
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    B, S, Hh, H = a.batch, 80000, 128, 128
    m = uvad_amd.PyanNet()                                                # 4 x 128 bidirectional, head 128 / 2, the reference's SincNet
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    T = m.num_frames(S)
    g = torch.Generator().manual_seed(1)
    wav = (0.1 * torch.randn(B, S, generator=g)).to(dev)
    y = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8).to(dev)
    L = m.hparams.lstm["num_layers"]

    hh, hl, hs = rt.head_train_open(), rt.lstm_train_open(layers=L), rt.sincnet_train_open()

    def step():
        f = rt.sincnet_train_forward(hs, wav)
        o = rt.lstm_train_forward(hl, f)
        _, gx = rt.head_train_grad(hh, o, y, want_grad_x=True)
        gin = rt.lstm_train_backward(hl, f, gx, want_grad_in=True)
        rt.sincnet_train_backward(hs, wav, gin)
        rt.head_train_apply(hh), rt.lstm_train_apply(hl), rt.sincnet_train_apply(hs)
        return gin
    gin = step().clone()                                                  # sizes the workspaces
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()

    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    P = {k[len("sincnet."):]: torch.nn.Parameter(v.clone().to(dev)) for k, v in sd.items() if k.startswith("sincnet.") and not k.endswith(("window_", "n_"))}
    lstm = torch.nn.LSTM(60, Hh, L, batch_first=True, bidirectional=True)
    lin = [torch.nn.Linear(2 * Hh, H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)]
    with torch.no_grad():
        for name, prm in lstm.named_parameters():
            prm.copy_(sd["lstm." + name])
        for i, mod in enumerate(lin):
            pre = f"linear.{i}" if i < 2 else "classifier"
            mod.weight.copy_(sd[pre + ".weight"]), mod.bias.copy_(sd[pre + ".bias"])
    lstm, lin = lstm.to(dev), [mod.to(dev) for mod in lin]
    opt = torch.optim.Adam(list(P.values()) + list(lstm.parameters()) + [p for mod in lin for p in mod.parameters()], lr=1e-3)
    yf = y.float()
    win, n_ = (torch.from_numpy(b).to(dev) for b in R.buffers())
    R.buffers = lambda: (win, n_)                                         # torch_filters reads them: keep them on the device

    def torch_filters(low_p, band_p):
        n = n_.view(1, -1)
        low = R.MIN_LOW + torch.abs(low_p)
        high = torch.clamp(low + R.MIN_BAND + torch.abs(band_p), R.MIN_LOW, R.RATE / 2)
        band = (high - low)[:, 0]
        fl, fh = torch.matmul(low, n), torch.matmul(high, n)
        cl = ((torch.sin(fh) - torch.sin(fl)) / (n / 2)) * win
        cos = torch.cat([cl, 2 * band.view(-1, 1), torch.flip(cl, dims=[1])], dim=1) / (2 * band[:, None])
        sl = ((torch.cos(fl) - torch.cos(fh)) / (n / 2)) * win
        sin = torch.cat([sl, torch.zeros_like(band.view(-1, 1)), -torch.flip(sl, dims=[1])], dim=1) / (2 * band[:, None])
        return torch.cat([cos, sin], dim=0).view(R.NF, 1, R.KS)
    R.torch_filters = lambda low_p, band_p, dtype: torch_filters(low_p, band_p)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        f, _ = R.torch_sincnet(P, wav)
        o, _ = lstm(f)
        o = torch.nn.functional.leaky_relu(lin[1](torch.nn.functional.leaky_relu(lin[0](o))))
        torch.nn.functional.binary_cross_entropy(torch.sigmoid(lin[2](o)).squeeze(-1), yf).backward()
        opt.step()

    cands = {"pyannet_train_graph": graph.replay, "torch_autograd_adam": torch_step,
             "phase_sincnet_forward": lambda: rt.sincnet_train_forward(hs, wav),
             "phase_sincnet_backward": lambda: rt.sincnet_train_backward(hs, wav, gin),
             "phase_sincnet_apply": lambda: rt.sincnet_train_apply(hs)}
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
    out = {"shape": {"B": B, "S": S, "T": T, "hidden": Hh, "directions": 2, "layers": L, "lin_hidden": H, "lin_layers": 2, "segment": "default (2048)"},
           "method": f"HIP events around blocks of {a.reps} calls, {a.blocks} blocks per candidate, candidates alternated block by block in one process; "
                     "the phases are eager calls of the runtime's wrappers (output allocation included), the step is one graph replay",
           "device": torch.cuda.get_device_name(0),
           "sincnet_workspace_bytes": int(rt.lib.uvad_sincnet_train_ws_bytes(rt.ctx, B, S)),
           "sincnet_state_bytes": int(rt.lib.uvad_sincnet_train_state_bytes(rt.ctx)),
           "sincnet_param_count": int(rt.lib.uvad_sincnet_train_param_count(rt.ctx))}
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()), "blocks_ms": [round(float(t), 4) for t in v]}
    out["ratio_to_torch"] = out["pyannet_train_graph"]["ms_median"] / out["torch_autograd_adam"]["ms_median"]
    out["ranges_resolve"] = bool(out["pyannet_train_graph"]["ms_min"] > out["torch_autograd_adam"]["ms_max"] or
                                 out["pyannet_train_graph"]["ms_max"] < out["torch_autograd_adam"]["ms_min"])
    out["sincnet_share_of_step"] = sum(out[k]["ms_median"] for k in ("phase_sincnet_forward", "phase_sincnet_backward", "phase_sincnet_apply")) / \
        out["pyannet_train_graph"]["ms_median"]
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
                      for k in list(cands) + ["ratio_to_torch", "ranges_resolve", "sincnet_share_of_step", "sincnet_workspace_bytes"]}))


if __name__ == "__main__":
    main()
