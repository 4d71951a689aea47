#!/usr/bin/env python3
"""Windowed streaming of a bidirectional PyanNet2 (uvad_window_step): B concurrent live feeds, `chunk` samples per step, the model run
from zero state over the last W frames every step, frames emitted L frames behind the newest complete one.
Reports p50/p99 wall latency per step (host submit -> logits visible after a synchronise), device time per step from HIP events and the
real-time factor (step wall time / audio time), timed only after the W-frame warm-up, for the step enqueued kernel by kernel and
replayed as a hipGraph.  In the same run it times the naive alternative: uvad_forward on the last W frames' worth of PCM (5 s at the
defaults) every step, from a torch-side ring."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.synth import seed_weights

ap = argparse.ArgumentParser()
ap.add_argument("--feeds", type=int, default=512)
ap.add_argument("--chunk", type=int, default=320)
ap.add_argument("--window", type=int, default=500)
ap.add_argument("--lookahead", type=int, default=50)
ap.add_argument("--seconds", type=float, default=60.0, help="audio per feed AFTER the warm-up")
ap.add_argument("--naive-steps", type=int, default=600)
args = ap.parse_args()
dev = torch.device("cuda:0")
F = 80
m = uvad_amd.PyanNet2(encoding_dim=F); m.build(); seed_weights(m, 1234, 2.0)              # bidirectional (LSTM_DEFAULTS)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type="hamming")); m = m.to(dev).eval()
rt = m.runtime(dev)
B, C, W, L = args.feeds, args.chunk, args.window, args.lookahead
shift = 160
warm = -(-(W * shift + 400) // C)                                                        # steps until the window is full
steps = int(args.seconds * 16000 / C)
g = torch.Generator(device=dev); g.manual_seed(5)
audio = 0.1 * torch.randn(B, 64 * C, generator=g, device=dev)                             # 64 distinct chunks, cycled
chunk_of = lambda i: audio[:, (i % 64) * C:(i % 64 + 1) * C].contiguous()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(step, n):
    lat, dev_ms, frames = [], [], 0
    for i in range(n):
        x = chunk_of(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = step(x)
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
        frames += out.shape[1]
    # a second, shorter pass with HIP events around the step (kept out of the latency loop)
    for i in range(min(n, 300)):
        x = chunk_of(i)
        torch.cuda.synchronize()
        e0.record()
        step(x)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    lat = np.array(lat) * 1e3
    audio_s = n * C / 16000.0
    return {"steps": n, "frames_per_feed": frames, "p50_ms": float(np.percentile(lat, 50)), "p99_ms": float(np.percentile(lat, 99)),
            "max_ms": float(lat.max()), "device_ms_p50": float(np.percentile(dev_ms, 50)), "rtf": float(lat.sum() / 1e3 / audio_s)}


res = {"config": f"{B} feeds x {C}-sample chunks, W = {W} frames, L = {L}, bidirectional PyanNet2 F = {F}, "
                 f"{steps * C / 16000.0:.0f} s of audio per feed timed after a {warm}-step warm-up"}
for graphs in (False, True):
    st = rt.window_stream_open(B, C, window=W, lookahead=L, graphs=graphs)
    for i in range(warm):
        rt.window_stream_step(st, chunk_of(i))
    torch.cuda.synchronize()
    r = timed(lambda x: rt.window_stream_step(st, x), steps)
    if graphs:
        r["graphs"] = len(st["graphs"])
    r["time_chunks"] = rt.time_chunks()
    res["window_graphs" if graphs else "window"] = r

# naive: the last W frames' worth of PCM in a torch-side ring, uvad_forward on all of it every step
S = W * shift
ring = torch.zeros(B, 2 * S, device=dev)
pos = [0]


def naive(x):
    p = pos[0] % S
    ring[:, p:p + C] = x[:, :min(C, S - p)]
    ring[:, p + S:p + S + C] = x[:, :min(C, S - p)]                       # mirrored copy: the last S samples are one contiguous slice
    if C > S - p:
        ring[:, :C - (S - p)] = x[:, S - p:]
        ring[:, S:S + C - (S - p)] = x[:, S - p:]
    pos[0] += C
    q = pos[0] % S
    lg, _ = rt.forward(ring[:, q:q + S], want_probs=False)
    return lg[:, -(C // shift + 1):]


for i in range(warm):
    naive(chunk_of(i))
torch.cuda.synchronize()
res["naive_forward_last_window"] = timed(naive, min(steps, args.naive_steps))
res["what"] = ("p50_ms = host wall time of one step (submit -> synchronised); device_ms = HIP events around the step; rtf = summed step wall "
               "time / audio time; naive = uvad_forward on the last W * shift samples every step (features of the whole window recomputed)")
print(json.dumps(res))
