#!/usr/bin/env python3
"""What scoring a batch on the device costs (uvad_score_step) against the path it replaces, at two shapes: 256 rows x 10 s
(T = 1000) and one 1-hour row (T = 360000), seeded probabilities and reference labels, one operating point (0.5, 49), 256 bins.
  (a) score   VadRuntime.score_step: two launches, nothing returns to the host;
  (b) torch   what a host loop does today: uvad_median_filter_lens + uvad_der_counts + F.binary_cross_entropy + torch.histc per class,
              ending in the .item() calls such a loop needs to accumulate.
The two alternate in blocks of --steps calls, --rounds times, in one process after --warmup calls of each; every call is timed with HIP
events (b: to the end of its last .item()) and a block reports its median.  Reported: the median over blocks, and the stage's share of a
`forward` step of the same batch (PyanNet2, 64 mels, bidirectional; 256 x 10 s only).  --out writes the JSON (profiles/score.json)."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.synth import seed_weights, synth_pcm_device

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100, help="calls per block")
ap.add_argument("--rounds", type=int, default=3, help="blocks of each setting, alternated")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--kernel", type=int, default=49)
ap.add_argument("--bins", type=int, default=256)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("run_score.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
rt = uvad_amd.VadRuntime(dev)


def timed(fn, n):
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def shape(B, T):
    g = torch.Generator(device=dev); g.manual_seed(3)
    probs = torch.rand((B, T), generator=g, device=dev)
    gt = ((torch.cumsum((torch.rand((B, T), generator=g, device=dev) < 0.01).to(torch.int32), 1) & 1) == 1).to(torch.uint8)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    sc = rt.score_open(points=[(0.5, args.kernel)], bins=args.bins)
    gtf = gt.to(torch.float32)
    tot = {"fa": 0, "md": 0, "loss": 0.0}

    def score():
        rt.score_step(sc, probs, gt, lengths=lens)

    def torch_path():
        pred = rt.median_filter(probs, args.kernel, lengths=lens)
        c = rt.der_counts(pred, gt).sum(0)
        loss = torch.nn.functional.binary_cross_entropy(probs, gtf, reduction="sum")
        h0 = torch.histc(probs[gt == 0], bins=args.bins, min=0.0, max=1.0)
        h1 = torch.histc(probs[gt == 1], bins=args.bins, min=0.0, max=1.0)
        tot["fa"] += int(c[0].item()); tot["md"] += int(c[1].item()); tot["loss"] += float(loss.item())
        tot["h"] = (h0.cpu(), h1.cpu())

    for fn in (score, torch_path):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    blocks = {"score": [], "torch": []}
    for _ in range(args.rounds):
        blocks["score"].append(timed(score, args.steps))
        blocks["torch"].append(timed(torch_path, args.steps))
    r = {"B": B, "T": T, "score_step_ms": float(np.median(blocks["score"])), "torch_path_ms": float(np.median(blocks["torch"])),
         "score_blocks_ms": blocks["score"], "torch_blocks_ms": blocks["torch"]}
    r["speedup"] = r["torch_path_ms"] / r["score_step_ms"]
    read = rt.score_read(sc)
    n = args.warmup + args.steps * args.rounds
    assert read["steps"] == n
    r["fa_frames_per_step"], r["md_frames_per_step"] = int(read["counts"][0][1]) // n, int(read["counts"][0][3]) // n
    r["agrees_with_torch_path"] = bool(int(read["counts"][0][1]) == tot["fa"] and int(read["counts"][0][3]) == tot["md"])
    return r


out = {"kernel": args.kernel, "bins": args.bins, "steps": args.steps, "rounds": args.rounds, "shapes": [shape(256, 1000), shape(1, 360000)]}
m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=64); m.build(); seed_weights(m, 1234, 2.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=64, window_type="hamming"))
m = m.to(dev).eval()
pcm = synth_pcm_device(256, 160000, seed=1, device=dev)
fwd = lambda: m.forward_waveform(pcm)
for _ in range(5):
    fwd()
torch.cuda.synchronize()
out["forward_256x10s_ms"] = timed(fwd, 30)
out["score_share_of_forward"] = out["shapes"][0]["score_step_ms"] / out["forward_256x10s_ms"]
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
