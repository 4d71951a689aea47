#!/usr/bin/env python3
"""The causal stream's slot pool (uvad_stream_slots_step) next to the lockstep step (uvad_stream_step), one run on one box: B slots of
`chunk` samples per step, causal PyanNet2 (F 64).  Four configurations, alternated block by block:
  lockstep   the lockstep group under its two graphs (stream_open(graphs=True); the tools/run_cfg5.py model and input)
  pool       the pool's one graph, every slot active
  churn      the pool under churn: about a quarter of the slots idle, sessions of U(1, 10) s starting and ending throughout
  chain      the churn pool with the hysteresis endpointer and the speech gate behind it, all in the one graph
Per configuration and block: the median host wall time of a step through VadRuntime (submit -> synchronised), the median of the graph
replay alone (chunk and flag bytes written to the fixed buffers before the clock starts) and the median device time from HIP events
around the replay.  Reported: the median over blocks, the block-to-block spread (max - min of the block medians) and the ratio to the
lockstep step; a difference below the two spreads is reported as not resolved.
--only-lockstep measures the first configuration alone; --root imports the package from another checkout (A/B against another revision
on one box: run the two alternately)."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--feeds", type=int, default=512)
ap.add_argument("--chunk", type=int, default=320)
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--steps", type=int, default=200, help="timed steps per block and configuration")
ap.add_argument("--only-lockstep", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import uvad_amd
from uvad_amd.synth import seed_weights

dev = torch.device("cuda:0")
m = uvad_amd.PyanNet2(lstm={"bidirectional": False}, encoding_dim=64); m.build(); seed_weights(m, 1234, 4.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=64, window_type="hamming")); m = m.to(dev).eval()
rt = m.runtime(dev)
B, CH = args.feeds, args.chunk
g = torch.Generator(device=dev); g.manual_seed(5)
audio = 0.1 * torch.randn(B, 64 * CH, generator=g, device=dev)        # 64 distinct chunks, cycled
chunk_of = lambda i: audio[:, (i % 64) * CH:(i % 64 + 1) * CH].contiguous()
total = args.blocks * args.steps * 3 + 64
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


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


class Lockstep:
    def __init__(self):
        self.st = rt.stream_open(B, CH, graphs=True)
        self.i = 0

    def call(self):
        x = chunk_of(self.i); self.i += 1
        return lambda: rt.stream_step(self.st, x)

    def replay(self):
        """The step's graph alone: the chunk is in the fixed buffer before the clock starts, the host counters move after it stops."""
        st = self.st
        self.after = None
        x = chunk_of(self.i); self.i += 1
        kk, off, par, first = C.c_int(), C.c_int64(), C.c_int(), C.c_int()
        rt._check(rt.lib.uvad_stream_peek(rt.ctx, st["state"].data_ptr(), CH, C.byref(kk), C.byref(off), C.byref(par), C.byref(first)))
        gr = st["graphs"].get((kk.value, off.value, par.value, first.value))
        if gr is None:
            return lambda: rt.stream_step(st, x)
        st["in"].copy_(x)

        def run():
            gr.replay()
        self.after = lambda: rt.lib.uvad_stream_advance(rt.ctx, st["state"].data_ptr(), CH)
        return run


class Pool:
    def __init__(self, churn, chain):
        kw = dict(endpoint={"onset": 0.6, "offset": 0.4, "min_on": 3, "min_off": 2}, gate={"max_len": 40}) if chain else {}
        self.st = rt.stream_slots_open(B, CH, graphs=True, **kw)
        self.i = 0
        rng = np.random.default_rng(7)
        f = np.zeros((total, B), np.uint8)
        if churn:      # sessions of U(1, 10) s with gaps of U(0, 3.7) s: about a quarter of the slots idle at any step
            for b in range(B):
                s = int(rng.integers(0, 40))
                while s < total:
                    n = int(rng.uniform(1, 10) * 16000 / CH)
                    f[s, b] |= 1
                    if s + n - 1 < total:
                        f[s + n - 1, b] |= 2
                    s += n + int(rng.uniform(0, 3.7) * 16000 / CH)
        else:
            f[0, :] = 1
        self.flags = f
        self.start = torch.from_numpy(f & 1 == 1).to(dev)
        self.end = torch.from_numpy(f & 2 == 2).to(dev)
        self.bytes = torch.from_numpy(f).to(dev)
        rt.stream_slots_step(self.st, chunk_of(0), start=self.start[0], end=self.end[0])      # captures the one graph
        self.i = 1

    def call(self):
        i = self.i; self.i += 1
        x = chunk_of(i)
        return lambda: rt.stream_slots_step(self.st, x, start=self.start[i], end=self.end[i])

    def replay(self):
        i = self.i; self.i += 1
        self.st["in"].copy_(chunk_of(i))
        self.st["flags"].copy_(self.bytes[i])
        return self.st["graph"].replay

    def idle_share(self):
        live, cur = np.zeros(self.flags.shape, bool), np.zeros(B, bool)
        for s in range(self.i):
            cur |= self.flags[s] & 1 == 1
            live[s] = cur
            cur &= ~(self.flags[s] & 2 == 2)
        return float(1.0 - live[1:self.i].mean())


cfgs = {"lockstep": Lockstep()}
if not args.only_lockstep:
    cfgs.update(pool=Pool(False, False), churn=Pool(True, False), chain=Pool(True, True))
for c in cfgs.values():                                                  # warm-up: every graph captured, every shape run
    for _ in range(24):
        c.call()()
torch.cuda.synchronize()
blocks = {k: {"call_ms": [], "replay_ms": [], "device_ms": []} for k in cfgs}
for blk in range(args.blocks):
    for name, c in cfgs.items():
        c.after = None
        call = [wall(c.call()) for _ in range(args.steps)]
        rep, dv = [], []
        for _ in range(args.steps):
            fn = c.replay()
            rep.append(wall(fn))
            if getattr(c, "after", None):
                c.after()
        for _ in range(args.steps):
            fn = c.replay()
            dv.append(dev_ms(fn))
            if getattr(c, "after", None):
                c.after()
        blocks[name]["call_ms"].append(float(np.median(call)))
        blocks[name]["replay_ms"].append(float(np.median(rep)))
        blocks[name]["device_ms"].append(float(np.median(dv)))


def summary(b):
    out = {}
    for k, v in b.items():
        out[k] = {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "blocks": [round(x, 5) for x in v]}
    return out


res = {"config": f"{B} slots x {CH}-sample chunks, causal PyanNet2 (F 64, 4 layers, 2 feed-forward layers); {args.blocks} blocks x {args.steps} steps per "
                 "measure and configuration, configurations alternated block by block",
       "what": "call_ms = host wall time of one step through VadRuntime (submit -> synchronised); replay_ms = the same around the graph replay "
               "alone; device_ms = HIP events around the replay; median over the block medians, spread = max - min of the block medians"}
for name, b in blocks.items():
    res[name] = summary(b)
if not args.only_lockstep:
    res["idle_share_under_churn"] = cfgs["churn"].idle_share()
    res["session_starts_under_churn"] = int((cfgs["churn"].flags[1:cfgs["churn"].i] & 1).sum())
    res["graphs"] = {"lockstep": len(cfgs["lockstep"].st["graphs"]), **{k: cfgs[k].st["graphs"] for k in ("pool", "churn", "chain")}}
    ratios = {}
    for name in ("pool", "churn", "chain"):
        for k in ("call_ms", "replay_ms", "device_ms"):
            a, b0 = res[name][k], res["lockstep"][k]
            resolved = abs(a["median"] - b0["median"]) > max(a["spread"], b0["spread"])
            ratios[f"{name}/{k}"] = {"ratio": a["median"] / b0["median"], "resolved": bool(resolved)}
    res["ratio_to_lockstep"] = ratios
print(json.dumps(res))
