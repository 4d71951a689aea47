"""Measure one graph replay of a full training step ending in uvad_optim_step (clipping, AdamW decay, a learning-rate table, the
non-finite skip) against the same step ending in the two _apply calls, at tools/run_lstm_train.py's shape: 256 x 1000 frames, hidden 128
bidirectional, one trainable layer, head 128 / 2.  One GPU, one run: HIP events around blocks of replays, the two graphs alternated block
by block, median and spread over the blocks.  The ends alone (the joint step's four kernels, the applies' four) are timed the same way as
eager calls on accumulators a backward call refilled before each block -- with an empty accumulator both return at once, so those two
figures include the refill's launch gap and are an upper bound.  Writes profiles/optim.json.
Usage: python tools/run_optim.py [--blocks 9] [--reps 10] [--out profiles/optim.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim.json"))
    a = ap.parse_args()
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    B, T, F = 256, 1000, 64
    m = uvad_amd.PyanNet2(encoding_dim=F)                                 # 4 x 128 bidirectional, head 128 / 2: the top layer and the head learn
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    g = torch.Generator().manual_seed(1)
    feats = (torch.randn(B, T, F, generator=g) * 2.0 - 3.0).to(dev)
    x_in = rt.lstm_train_input(feats, layers=1).clone()                   # the frozen three layers' output, cached
    y = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8).to(dev)
    table = [1e-3 * min(1.0, (t + 1) / 100.0) for t in range(1000)]
    cfg = {"max_norm": 1.0, "weight_decay": 1e-2, "adamw": True, "skip_nonfinite": True}

    def handles():
        hh, hl = rt.head_train_open(), rt.lstm_train_open(layers=1)
        out_y = rt.lstm_train_forward(hl, x_in)                           # sizes the workspaces
        _, gx = rt.head_train_grad(hh, out_y, y, want_grad_x=True)
        rt.lstm_train_backward(hl, x_in, gx)
        return hh, hl, out_y, gx
    ah, al, out_y, gx = handles()
    oh, ol, _, _ = handles()
    o = rt.optim_open(cfg, table)
    rt.head_train_apply(ah), rt.lstm_train_apply(al)
    rt.optim_step(o, head=oh, lstm=ol)
    torch.cuda.synchronize()

    def step(hh, hl, end):
        out = rt.lstm_train_forward(hl, x_in)
        _, gxx = rt.head_train_grad(hh, out, y, want_grad_x=True)
        rt.lstm_train_backward(hl, x_in, gxx)
        end()
    graphs = {}
    for name, hh, hl, end in (("step_apply_graph", ah, al, lambda: (rt.head_train_apply(ah), rt.lstm_train_apply(al))),
                              ("step_optim_graph", oh, ol, lambda: rt.optim_step(o, head=oh, lstm=ol))):
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            step(hh, hl, end)

    def refill(hh, hl):
        rt.head_train_grad(hh, out_y, y, want_grad_x=False)
        rt.lstm_train_backward(hl, x_in, gx)

    def end_apply():
        refill(ah, al)
        rt.head_train_apply(ah), rt.lstm_train_apply(al)

    def end_optim():
        refill(oh, ol)
        rt.optim_step(o, head=oh, lstm=ol)
    cands = {"step_apply_graph": graphs["step_apply_graph"].replay, "step_optim_graph": graphs["step_optim_graph"].replay,
             "refill_only": lambda: refill(ah, al), "refill_and_applies": end_apply, "refill_and_optim_step": end_optim}
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
    rec = rt.optim_read(o)
    out = {"shape": {"B": B, "T": T, "hidden": 128, "directions": 2, "trainable_layers": 1, "lin_hidden": 128, "lin_layers": 2, "segment": "default (2048)"},
           "options": dict(cfg, lr_table="1000 entries, linear warmup over 100"),
           "method": f"HIP events around blocks of {a.reps} calls, {a.blocks} blocks per candidate, candidates alternated block by block in one process; "
                     "the two steps are graph replays; the refill_* candidates are eager calls (head grad + LSTM backward refill the accumulators, "
                     "then the end under test): their difference to refill_only bounds the end's cost from above",
           "device": torch.cuda.get_device_name(0),
           "head_param_count": int(rt.lib.uvad_head_train_param_count(rt.ctx)), "lstm_param_count": int(rt.lib.uvad_lstm_train_param_count(rt.ctx)),
           "optim_workspace_bytes": int(rt.lib.uvad_optim_ws_bytes(rt.ctx)), "optim_steps_applied": rec["step"], "optim_steps_skipped": rec["skipped"]}
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()), "blocks_ms": [round(float(t), 4) for t in v]}
    s, q = out["step_apply_graph"], out["step_optim_graph"]
    out["step_difference_ms"] = q["ms_median"] - s["ms_median"]
    out["ranges_resolve"] = bool(q["ms_min"] > s["ms_max"] or q["ms_max"] < s["ms_min"])
    out["end_applies_ms"] = out["refill_and_applies"]["ms_median"] - out["refill_only"]["ms_median"]
    out["end_optim_step_ms"] = out["refill_and_optim_step"]["ms_median"] - out["refill_only"]["ms_median"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (out[k]["ms_median"] if isinstance(out[k], dict) and "ms_median" in out[k] else out[k])
                      for k in list(cands) + ["step_difference_ms", "ranges_resolve", "end_applies_ms", "end_optim_step_ms", "optim_steps_applied"]}))


if __name__ == "__main__":
    main()
