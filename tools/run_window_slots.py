#!/usr/bin/env python3
"""Slot pools under churn (uvad_window_slots_step / uvad_window_wav_slots_step_i16): B slots of `chunk` samples per step, sessions of
seeded U(2, 30) s lengths starting and ending throughout, every step replayed from the one captured graph.  Alternated step by step in
the same run: the existing window stream group (uvad_window_step / uvad_window_wav_step_i16) at the same (B, chunk, W, L), all feeds
started together, no churn, its steady-state graphs replayed.
Reports p50/p99 wall latency per step (host submit -> outputs visible after a synchronise), device time per step from HIP events, the
real-time factor (step wall time / audio time) and the slot / group ratio; and the warm-up at T = W: the pool's first steps (every slot
starting at once, one graph) next to the group's eager warm-up steps.  --family logmel (PyanNet2, W 500, L 50) or wav (PyanNet, int16,
W 293, L 30).  What the new kernels cost comes from a kernel trace of a short run (profiles/README.md)."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.synth import seed_weights

ap = argparse.ArgumentParser()
ap.add_argument("--family", choices=["logmel", "wav"], default="logmel")
ap.add_argument("--feeds", type=int, default=512)
ap.add_argument("--chunk", type=int, default=320)
ap.add_argument("--window", type=int, default=0, help="0: 500 (logmel) / 293 (wav)")
ap.add_argument("--lookahead", type=int, default=-1, help="-1: 50 (logmel) / 30 (wav)")
ap.add_argument("--steps", type=int, default=1500, help="timed steps of each (pool and group, alternated)")
ap.add_argument("--profile", action="store_true", help="a short run for a kernel trace: no timing loops")
args = ap.parse_args()
dev = torch.device("cuda:0")
wav = args.family == "wav"
B, C = args.feeds, args.chunk
W = args.window or (293 if wav else 500)
L = args.lookahead if args.lookahead >= 0 else (30 if wav else 50)
if wav:
    torch.manual_seed(11)
    m = uvad_amd.PyanNet(); m.build(); seed_weights(m, 1234, 2.0)
else:
    m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=64); m.build(); seed_weights(m, 1234, 2.0)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=64))
m = m.to(dev).eval()
rt = m.runtime(dev)
g = torch.Generator(device=dev); g.manual_seed(5)
audio = 0.1 * torch.randn(B, 64 * C, generator=g, device=dev)                             # 64 distinct chunks, cycled
if wav:
    audio = torch.round(audio * 32767.0).clamp(-32768, 32767).to(torch.int16)
chunk_of = lambda i: audio[:, (i % 64) * C:(i % 64 + 1) * C].contiguous()
if wav:
    J, R = rt.wav_window_geometry()
    warm = -(-(R + J * (W - 1) + J) // C)                                                 # steps until the window is full
else:
    warm = -(-(W * 160 + 400) // C)

# churn: per slot, sessions of U(2, 30) s back to back with gaps of 0 .. 0.4 s; the pool's first steps start every slot at once
rng = np.random.default_rng(7)
total = warm + 2 * args.steps + 8
starts, ends = np.zeros((total, B), bool), np.zeros((total, B), bool)
for b in range(B):
    s = 0
    while s < total:
        n = int(rng.uniform(2, 30) * 16000 / C)
        starts[s, b] = True
        if s + n - 1 < total:
            ends[s + n - 1, b] = True
        s += n + int(rng.integers(0, 20))
flags = torch.from_numpy(starts.astype(np.uint8) | (ends.astype(np.uint8) << 1)).to(dev)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

if wav:
    pool = rt.wav_window_slots_open(B, C, window=W, lookahead=L, graphs=True, dtype=torch.int16)
    group = rt.wav_window_stream_open(B, C, window=W, lookahead=L, graphs=True, dtype=torch.int16)
    pool_step = lambda i, x: rt.wav_window_slots_step(pool, x, start=flags[i] & 1 == 1, end=flags[i] & 2 == 2)
    group_step = lambda x: rt.wav_window_stream_step(group, x)
else:
    pool = rt.window_slots_open(B, C, window=W, lookahead=L, graphs=True)
    group = rt.window_stream_open(B, C, window=W, lookahead=L, graphs=True)
    pool_step = lambda i, x: rt.window_slots_step(pool, x, start=flags[i] & 1 == 1, end=flags[i] & 2 == 2)
    group_step = lambda x: rt.window_stream_step(group, x)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def dev_ms(fn):
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


# warm-up at T = W: the pool (all slots start on step 0; one graph from the first step on) and the group (eager until the window is full)
pool_warm = [wall(lambda i=i: pool_step(i, chunk_of(i))) for i in range(warm)]
group_warm = [wall(lambda i=i: group_step(chunk_of(i))) for i in range(warm)]
if args.profile:
    for i in range(warm, warm + 40):
        pool_step(i, chunk_of(i)); group_step(chunk_of(i))
    torch.cuda.synchronize()
    print(json.dumps({"profile_run": True, "steps": warm + 40}))
    sys.exit(0)
lat_p, lat_g, dev_p, dev_g = [], [], [], []
i = warm
for k in range(args.steps):
    x = chunk_of(i)
    if k % 5 == 4:   # every fifth pair timed with HIP events instead
        dev_p.append(dev_ms(lambda: pool_step(i, x)))
        dev_g.append(dev_ms(lambda: group_step(x)))
    else:
        lat_p.append(wall(lambda: pool_step(i, x)))
        lat_g.append(wall(lambda: group_step(x)))
    i += 1
lat_p, lat_g = np.array(lat_p), np.array(lat_g)
audio_ms = C / 16.0


def summary(lat, dv):
    return {"p50_ms": float(np.percentile(lat, 50)), "p99_ms": float(np.percentile(lat, 99)), "max_ms": float(lat.max()),
            "device_ms_p50": float(np.percentile(dv, 50)), "rtf": float(lat.mean() / audio_ms)}


n_starts = int(starts[warm:i].sum())
res = {"config": f"{B} {'int16' if wav else 'f32'} {'PyanNet' if wav else 'PyanNet2 (bidirectional, F 64)'} slots x {C}-sample chunks, "
                 f"W = {W}, L = {L}; {len(lat_p) + len(dev_p)} timed steps of each, alternated, after a {warm}-step warm-up",
       "pool_under_churn": summary(lat_p, dev_p), "group_no_churn": summary(lat_g, dev_g),
       "session_starts_in_timed_steps": n_starts, "pool_graphs": pool["graphs"],
       "group_graphs": len(group["graphs"]),
       "warmup_T_eq_W": {"steps": warm, "pool_ms_total": float(np.sum(pool_warm)), "pool_ms_p50": float(np.median(pool_warm[1:])),
                         "group_eager_ms_total": float(np.sum(group_warm)), "group_eager_ms_p50": float(np.median(group_warm[1:]))},
       "time_chunks": rt.time_chunks()}
res["slot_over_group_p50"] = res["pool_under_churn"]["p50_ms"] / res["group_no_churn"]["p50_ms"]
res["slot_over_group_device"] = res["pool_under_churn"]["device_ms_p50"] / res["group_no_churn"]["device_ms_p50"]
res["what"] = ("p50_ms = host wall time of one step (submit -> synchronised); device_ms = HIP events around the step; rtf = mean step wall "
               "time / audio time per step; warm-up: the pool's first W-frame steps (the first one captures its graph) next to the group's "
               "eager warm-up steps")
print(json.dumps(res))
