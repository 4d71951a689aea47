#!/usr/bin/env python3
"""Measurements of sliding-window inference over whole recordings (profiles/sliding.json).

One int16 recording of --minutes (default 60) of synthetic speech, window 5 s (W = 500 frames):
  --what predict   predict_vad end to end (wav file -> intervals) at hop_seconds None (the disjoint cuts), 5.0, 2.5 and 0.5, host wall time,
                   median of --calls after one warm-up call each; VadRuntime.sliding_forward alone on the device-resident recording at the
                   same hops (synchronise, call, synchronise); and the naive composition of existing calls -- fbank, torch unfold,
                   uvad_classify in batches of --group windows, torch index_add aggregation (full windows only) -- at the same hops.
  --what profile   a short run for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/run_sliding.py --what profile): a few
                   sliding_forward calls at --hop, no timing.
  --what share     --kernel-stats <kernel_stats.csv of that trace>: the share of the traced kernel time spent in the sliding_* kernels.
"""
import argparse, csv, json, os, sys, tempfile, time, wave
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=["predict", "profile", "share"], required=True)
ap.add_argument("--minutes", type=float, default=60.0)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--hop", type=float, default=2.5)
ap.add_argument("--group", type=int, default=512, help="windows per classifier launch")
ap.add_argument("--kernel-stats", default="")
args = ap.parse_args()

if args.what == "share":
    import re
    rows = list(csv.DictReader(line for line in open(args.kernel_stats) if not line.startswith("#")))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    mine = {}
    for r in rows:
        k = re.search(r"sliding_\w+", r["Name"])
        if k:
            mine[k.group(0)] = mine.get(k.group(0), 0.0) + float(r["TotalDurationNs"])
    print(json.dumps({"traced_kernel_ms": total * 1e-6, "sliding_kernels_ms": {k: v * 1e-6 for k, v in mine.items()},
                      "sliding_share": sum(mine.values()) / total}))
    sys.exit(0)

import torch
import uvad_amd
from uvad_amd.postprocess import sliding_weights
from uvad_amd.synth import seed_weights, synth_pcm

dev = torch.device("cuda:0")
SR, W, F = 16000, 500, 64
minute = np.round(synth_pcm(1, 60 * SR, seed=77)[0] * 32767.0).astype(np.int16)
pcm16 = np.tile(minute, int(np.ceil(args.minutes)))[:int(args.minutes * 60 * SR)]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fn, calls):
    fn()
    return float(np.median([wall_ms(fn)[0] for _ in range(calls)]))


m = uvad_amd.PyanNet2(encoding_dim=F); m.build(); seed_weights(m, 1234, 2.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=F))
m = m.to(dev).eval()
rt = m.runtime(dev)
x = torch.from_numpy(pcm16).to(dev)[None]
S = x.shape[1]

if args.what == "profile":
    Hf = int(round(args.hop * 100))
    rt.sliding_configure(W, Hf, sliding_weights("hamming", W))
    for _ in range(3):
        rt.sliding_forward(x, [S], group=args.group)
    torch.cuda.synchronize()
    print(json.dumps({"profile_run": True, "hop_frames": Hf}))
    sys.exit(0)

from config.config import load_config
from src.scripts import predict_vad

res = {"recording_minutes": args.minutes, "group": args.group, "frames": rt.num_frames(S), "window_frames": W, "calls": args.calls,
       "what": "predict_vad_ms: host wall time of predict_vad on one int16 wav file (read, upload, model, post-processing, one warm-up call "
               "first); sliding_forward_ms: VadRuntime.sliding_forward on the device-resident recording (synchronise, call, synchronise); "
               "naive_ms: fbank + torch unfold + uvad_classify in batches of --group + torch index_add aggregation, full windows only; medians"}
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "hour.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm16.tobytes())
    cfg = load_config()
    cfg.model_dict.encoding_dim = F
    cfg.weights_scale = 2.0
    cfg.max_duration = 2 * args.minutes * 60
    cfg.input.kind = "wav"
    cfg.input.paths = [path]
    cfg.sliding_group = args.group
    res["predict_vad_ms"] = {}
    for hop in (None, 5.0, 2.5, 0.5):
        cfg.hop_seconds = hop
        res["predict_vad_ms"][str(hop)] = median_ms(lambda: predict_vad(**cfg), args.calls)

res["sliding_forward_ms"], res["naive_ms"], res["windows"] = {}, {}, {}
for hop in (5.0, 2.5, 0.5):
    Hf = int(round(hop * 100))
    wts = sliding_weights("hamming", W)
    rt.sliding_configure(W, Hf, wts)
    res["sliding_forward_ms"][str(hop)] = median_ms(lambda: rt.sliding_forward(x, [S], group=args.group), args.calls)
    res["windows"][str(hop)] = int(rt.lib.uvad_sliding_count(rt.num_frames(S), W, Hf))
    wt = torch.from_numpy(wts).to(dev)

    def naive():
        feats = rt.fbank(x)                                                   # (1, T, F)
        T = feats.shape[1]
        wins = feats[0].unfold(0, W, Hf).permute(0, 2, 1).contiguous()        # (n, W, F), full windows only
        num, den = torch.zeros(T, device=dev), torch.zeros(T, device=dev)
        idx = (torch.arange(wins.shape[0], device=dev)[:, None] * Hf + torch.arange(W, device=dev)[None]).reshape(-1)
        for i in range(0, wins.shape[0], args.group):
            _, p = rt.classify(wins[i:i + args.group], want_logits=False)
            num.index_add_(0, idx[i * W:(i + p.shape[0]) * W], (p * wt).reshape(-1))
            den.index_add_(0, idx[i * W:(i + p.shape[0]) * W], wt.repeat(p.shape[0]))
        return num / den.clamp_min(1e-30)

    res["naive_ms"][str(hop)] = median_ms(naive, args.calls)
base = res["sliding_forward_ms"]["5.0"]
res["cost_ratio_vs_hop_equals_window"] = {k: v / base for k, v in res["sliding_forward_ms"].items()}
print(json.dumps(res))
