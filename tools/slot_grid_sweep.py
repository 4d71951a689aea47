#!/usr/bin/env python3
"""Persistent-grid sizes with several steps in flight: bench.py's workload (256 x 10 s, throughput recurrence) on one ForwardPipeline,
timed with uvad_set_concurrent_steps forced to each value of --settings on every slot, whatever the depth -- at 256 CUs and the
flagship's 32-CU recurrence launches 1 / 3 / 5 / 7 give projection grids of 256 / 192 / 128 / 64.  The settings are timed in turn,
--rounds times over, in one process on one box (profiles/slot_grid.json).

    python tools/slot_grid_sweep.py --depth 3 [--queues 16] [--settings 1,3,5,7] [--steps 200] [--rounds 3] [--out FILE]

--queues sets GPU_MAX_HW_QUEUES for this process (before the HIP runtime starts): depth 12 needs 16."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--depth", type=int, default=3)
ap.add_argument("--queues", type=int, default=0)
ap.add_argument("--settings", default="1,3,5,7")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--settle", type=float, default=0.4)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.queues:
    os.environ["GPU_MAX_HW_QUEUES"] = str(args.queues)

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.synth import seed_weights, synth_pcm_device

dev = torch.device("cuda:0")
B, S, F = 256, 160000, 64
model = uvad_amd.PyanNet2(encoding_dim=F)
model.build()
seed_weights(model, 1234, 4.0)
model.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type="hamming"))
model = model.to(dev).eval()
pipe = uvad_amd.ForwardPipeline(model, dev, depth=args.depth, recurrent_tile=16)
pcm = synth_pcm_device(B, S, seed=42, device=dev)
T = pipe.runtimes[0].num_frames(S)
for r in pipe.runtimes:
    r.forward(pcm, want_probs=False)
torch.cuda.synchronize(dev)


def run(n):
    for r in pipe.runtimes:
        r.set_concurrent_steps(n)
    t_s = time.perf_counter()
    keep = []
    while time.perf_counter() - t_s < args.settle:     # untimed: the clock the regime sustains (bench.py does the same)
        keep.append(pipe.submit(pcm))
        if len(keep) > args.depth:
            keep.pop(0).wait()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pipe.submit(pcm)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    return pipe.runtimes[0].projection_grid(), dt / args.steps * 1e3


settings = [int(x) for x in args.settings.split(",")]
res = {n: {"grid": None, "ms_per_step": []} for n in settings}
for _ in range(args.rounds):
    for n in settings:
        g, ms = run(n)
        res[n]["grid"] = g
        res[n]["ms_per_step"].append(round(ms, 4))
out = {"depth": args.depth, "queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": args.steps, "frames_per_step": B * T,
       "by_concurrent_steps": {str(n): dict(v, M_frames_per_s=[round(B * T / m / 1e3, 2) for m in v["ms_per_step"]]) for n, v in res.items()}}
text = json.dumps(out, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
pipe.close()
