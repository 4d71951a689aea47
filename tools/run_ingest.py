#!/usr/bin/env python3
"""The ingest stage's measurements (profiles/ingest.json).

  --what dense    the dense ingest kernel at 256 rows x 10 s of 8 kHz two-channel mu-law (512 x 160 000 output samples): HIP-event time per
                  call over a batch of calls, and achieved bytes/s against the kernel's algorithmic bytes (1 B read per input sample, 4 B
                  written per output sample).  The kernel's own time comes from a kernel trace of --profile (profiles/README.md).
  --what child    one process, one library: median wall time of (a) forward on a 512 x 160 000 f32 batch -- with --ingest:
                  forward(ingest(x)) from the 8 kHz two-channel mu-law source of the same shape -- and (b) the waveform slot pool step at
                  512 feeds x 20 ms replayed from its graph -- with --ingest: ingest_step + wav_window_slots_step, both from graphs, fed
                  8 kHz mu-law.  --lib runs another build of the library (the parent commit's, which has no ingest stage).
  --what ab       alternates child processes, this tree with --ingest against --parent-lib without, --rounds times on one box, and applies
                  the gates: median(with ingest) <= median(parent) + the ingest kernel's time + the parent's own spread (max - min of its
                  rounds).  The ingest kernel's time: the dense call's from --kernel-stats (the kernel trace's stats csv of
                  --what dense --profile) or --kernel-us; the step's own time is what the children measure (the replay of the captured
                  ingest step between two HIP events).  Exit status 1 if a gate fails.
"""
import argparse, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=["dense", "child", "ab"], required=True)
ap.add_argument("--lib", default="")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--ingest", action="store_true")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--kernel-us", type=float, default=0.0)
ap.add_argument("--kernel-stats", default="", help="kernel_stats.csv of a trace of --what dense --profile: the ingest kernel's average time")
ap.add_argument("--profile", action="store_true", help="a short run for a kernel trace: no timing loops")
args = ap.parse_args()

if args.what == "ab":
    me = os.path.abspath(__file__)
    runs = {"ingest": [], "parent": []}
    for r in range(args.rounds):
        for name, extra in (("parent", ["--lib", args.parent_lib]), ("ingest", ["--ingest"])):
            out = subprocess.run([sys.executable, me, "--what", "child", "--calls", str(args.calls), "--steps", str(args.steps)] + extra,
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                sys.exit(f"child ({name}, round {r}) failed with {out.returncode}:\n{out.stderr[-3000:]}")   # nothing more runs on the GPU
            runs[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
    kernel_us = args.kernel_us
    if args.kernel_stats:
        import csv
        rows = [r for r in csv.DictReader(open(args.kernel_stats)) if "ingest_kernel" in r["Name"]]
        kernel_us = sum(float(r["TotalDurationNs"]) for r in rows) / sum(int(r["Calls"]) for r in rows) * 1e-3
    step_us = float(np.median([x["ingest_step_replay_ms"] for x in runs["ingest"]])) * 1e3
    res = {"rounds": args.rounds, "runs": runs,
           "replay_allocations": [x["replay_allocations"] for x in runs["ingest"]],
           "what": "forward_ms: host wall time (synchronise, call, synchronise) of forward on 512 x 160 000 f32 (parent library) against "
                   "forward(ingest(x)) from 256 x 80 000 x 2 mu-law at 8 kHz (this tree), median of the calls of a process; step_ms: the same "
                   "for wav_window_slots_step at 512 x 320 f32 (parent) against ingest_step + wav_window_slots_step from 512 x 160 mu-law, all "
                   "replayed from graphs; gate: with-ingest median <= parent median + ingest kernel time + parent spread (max - min of its rounds); "
                   "replay_allocations: allocator calls during 200 replays of the captured ingest step under torch's sync debug mode 'error'"}
    for key, kern in (("forward_ms", kernel_us), ("step_ms", step_us)):
        a = np.array([x[key] for x in runs["ingest"]]); p = np.array([x[key] for x in runs["parent"]])
        spread = float(p.max() - p.min())
        limit = float(np.median(p)) + kern * 1e-3 + spread
        res[key] = {"with_ingest_median": float(np.median(a)), "parent_median": float(np.median(p)), "ingest_kernel_ms": kern * 1e-3,
                    "parent_spread_ms": spread, "limit_ms": limit, "gate_passed": bool(np.median(a) <= limit)}
    print(json.dumps(res))
    sys.exit(0 if res["forward_ms"]["gate_passed"] and res["step_ms"]["gate_passed"] else 1)

import torch
import uvad_amd
from uvad_amd import _lib
from uvad_amd.synth import seed_weights
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
    if not args.ingest:   # a build without the ingest stage: bind what it has (a missing symbol is otherwise a loud error, by design)
        for k in [k for k in _lib.SIGNATURES if k.startswith("uvad_ingest")]:
            del _lib.SIGNATURES[k]
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev); gen.manual_seed(5)


def ulaw(shape):
    return torch.randint(0, 256, shape, generator=gen, device=dev, dtype=torch.uint8)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


if args.what == "dense":
    from uvad_amd.runtime import VadRuntime
    rt = VadRuntime(dev)
    rt.ingest_configure("ulaw", 2, 8000)
    B, S = 256, 80000
    x = ulaw((B, S, 2))
    for _ in range(3):
        y = rt.ingest(x)
    torch.cuda.synchronize()
    if args.profile:
        print(json.dumps({"profile_run": True}))
        sys.exit(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = torch.empty_like(y)
    lib, ctx, st = rt.lib, rt.ctx, rt._stream()
    per = []
    for _ in range(10):
        e0.record()
        for _ in range(20):
            lib.uvad_ingest(ctx, x.data_ptr(), B, S, out.data_ptr(), st)
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / 20)
    nbytes = x.numel() + 4 * y.numel()
    ms = float(np.median(per))
    print(json.dumps({"config": f"{B} rows x {S} frames of 8 kHz two-channel mu-law -> {y.shape[0]} x {y.shape[1]} f32",
                      "algorithmic_bytes": nbytes, "event_ms_per_call_median_of_10x20": ms, "event_ms_min": float(min(per)),
                      "bytes_per_s": nbytes / (ms * 1e-3), "fraction_of_8TBps": nbytes / (ms * 1e-3) / 8e12,
                      "what": "back-to-back calls between two HIP events (includes launch gaps); the kernel's own time is in the kernel trace"}))
    sys.exit(0)

# ---- child: forward at 512 x 160 000 and the waveform slot pool step at 512 x 20 ms, one library
res = {"lib": _lib.LIB_PATH, "ingest": args.ingest}
m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=64); m.build(); seed_weights(m, 1234, 2.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=64))
m = m.to(dev).eval()
rt = m.runtime(dev)
if args.ingest:
    rt.ingest_configure("ulaw", 2, 8000)
    src = ulaw((256, 80000, 2))
    buf = torch.empty((512, 160000), dtype=torch.float32, device=dev)
    call = lambda: rt.forward(rt.ingest(src, out=buf))
else:
    pcm = 0.1 * torch.randn(512, 160000, generator=gen, device=dev)
    call = lambda: rt.forward(pcm)
for _ in range(5):
    call()
if not args.profile:
    res["forward_ms"] = float(np.median([wall_ms(call) for _ in range(args.calls)]))

torch.manual_seed(11)
mw = uvad_amd.PyanNet(); mw.build(); seed_weights(mw, 1234, 2.0)
mw = mw.to(dev).eval()
rtw = mw.runtime(dev)
B, W, L = 512, 293, 30
pool = rtw.wav_window_slots_open(B, 320, window=W, lookahead=L, graphs=True, dtype=torch.float32)
start = torch.ones(B, dtype=torch.bool, device=dev)
if args.ingest:
    rtw.ingest_configure("ulaw", 1, 8000)
    ing = rtw.ingest_open(B, 160, graphs=True)
    feed = ulaw((B, 64 * 160, 1))
    step = lambda i: rtw.wav_window_slots_step(pool, rtw.ingest_step(ing, feed[:, (i % 64) * 160:(i % 64 + 1) * 160]), start=start if i == 0 else None)
else:
    feed = 0.1 * torch.randn(B, 64 * 320, generator=gen, device=dev)
    step = lambda i: rtw.wav_window_slots_step(pool, feed[:, (i % 64) * 320:(i % 64 + 1) * 320], start=start if i == 0 else None)
warm = 260                                                    # the window (293 frames of 270 samples) is full after 250 steps
for i in range(warm):
    step(i)
torch.cuda.synchronize()
if args.profile:
    for i in range(warm, warm + 20):
        step(i)
    torch.cuda.synchronize()
    print(json.dumps({"profile_run": True}))
    sys.exit(0)
lat = [wall_ms(lambda i=i: step(i)) for i in range(warm, warm + args.steps)]
res["step_ms"] = float(np.median(lat))
res["step_ms_p99"] = float(np.percentile(lat, 99))
res["pool_graphs"] = pool["graphs"]
if args.ingest:
    res["ingest_graphs"] = ing["graphs"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    alloc0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")                   # a host synchronisation inside a replay raises
    e0.record()
    for _ in range(200):
        ing["graph"].replay()
    e1.record()
    torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    res["ingest_step_replay_ms"] = e0.elapsed_time(e1) / 200
    res["replay_allocations"] = torch.cuda.memory_stats(dev)["allocation.all.allocated"] - alloc0
print(json.dumps(res))
