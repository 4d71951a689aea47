#!/usr/bin/env python3
"""What the live endpointer (uvad_endpoint_step) adds to a slot pool step: 512 feeds x 20 ms, the step replayed from its one
captured graph with and without the endpoint node (window_slots_open / wav_window_slots_open, endpoint={"kernel": 25, "pad": 10}), sessions
of seeded U(2, 30) s lengths starting and ending throughout as in tools/run_window_slots.py.  The two settings alternate in blocks of
--steps replays, --rounds times, in one process; every step is timed with HIP events and a block reports its median.  Reported: the
median over blocks of each setting, the added time per step and its fraction of the step; and the host alternative the node replaces,
timed on the same probabilities: copying the step's [B][ld_out] probabilities and counts to the host and walking 512 Python / numpy
endpointers.  --family logmel (PyanNet2, W 500, L 50) or wav (PyanNet, int16, W 293, L 30).  The kernel's own duration comes from a kernel
trace of a short run (--profile; profiles/README.md)."""
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
ap.add_argument("--kernel", type=int, default=25)
ap.add_argument("--pad", type=int, default=10)
ap.add_argument("--steps", type=int, default=200, help="replays per block")
ap.add_argument("--rounds", type=int, default=3, help="blocks of each setting, alternated")
ap.add_argument("--host-steps", type=int, default=40, help="steps of the host alternative")
ap.add_argument("--profile", action="store_true", help="a short run for a kernel trace: no timing loops")
args = ap.parse_args()
dev = torch.device("cuda:0")
wav = args.family == "wav"
B, C, K, P = args.feeds, args.chunk, args.kernel, args.pad
W, L = (293, 30) if wav else (500, 50)
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

# churn: per slot, sessions of U(2, 30) s back to back with gaps of 0 .. 0.4 s; both pools walk the same schedule, each at its own step
rng = np.random.default_rng(7)
total = warm + args.steps * args.rounds + args.host_steps + 80
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

ep_cfg = {"kernel": K, "pad": P}
if wav:
    opener = lambda ep: rt.wav_window_slots_open(B, C, window=W, lookahead=L, graphs=True, dtype=torch.int16, endpoint=ep)
    stepper = rt.wav_window_slots_step
else:
    opener = lambda ep: rt.window_slots_open(B, C, window=W, lookahead=L, graphs=True, endpoint=ep)
    stepper = rt.window_slots_step
pools = {"without": opener(None), "with": opener(ep_cfg)}
at = {"without": 0, "with": 0}


def step(name):
    i = at[name]
    stepper(pools[name], chunk_of(i), start=flags[i] & 1 == 1, end=flags[i] & 2 == 2)
    at[name] = i + 1


for name in pools:                                                                        # warm-up until every window is full
    for _ in range(warm):
        step(name)
torch.cuda.synchronize()
if args.profile:
    for _ in range(60):
        step("with")
    torch.cuda.synchronize()
    print(json.dumps({"profile_run": True, "steps": warm + 60}))
    sys.exit(0)

e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def replay_ms(name):
    """Device time of the graph replay alone (the chunk and flag copies in front of it are the same in both settings)."""
    pool = pools[name]
    i = at[name]
    pool["in"].copy_(chunk_of(i))
    pool["flags"].copy_(flags[i])
    torch.cuda.synchronize()
    e0.record()
    pool["graph"].replay()
    e1.record()
    torch.cuda.synchronize()
    at[name] = i + 1
    return e0.elapsed_time(e1)


blocks = {"without": [], "with": []}
for r in range(args.rounds):
    for name in (("without", "with") if r % 2 == 0 else ("with", "without")):
        blocks[name].append(float(np.median([replay_ms(name) for _ in range(args.steps)])))


# the host alternative: probabilities and counts to the host every step, 512 endpointers in Python (last 2 h labels' inputs kept per feed)
class HostSlot:
    def __init__(self):
        self.x, self.m, self.fin, self.state, self.c = np.zeros(0, np.uint8), 0, 0, 0, 0

    def step(self, p, fl):
        h = K // 2
        if fl & 1:
            self.__init__()
        self.x = np.concatenate((self.x, ~(p < 0.5)))
        base = self.m - (len(self.x) - len(p))                                            # frame of x[0]
        self.m += len(p)
        upto = self.m if fl & 2 else max(0, self.m - h)
        ev = []
        if upto > self.fin:
            cs = np.concatenate(([0], np.cumsum(self.x, dtype=np.int64)))
            t = np.arange(self.fin, upto)
            y = cs[np.minimum(t + h + 1, self.m) - base] - cs[np.maximum(t - h, base) - base] > h
            for tt, v in zip(t.tolist(), y.tolist()):
                if self.state == 0 and v:
                    ev.append((1, max(tt - P, 0))); self.state = 1
                elif self.state == 1 and not v:
                    self.state, self.c = 2, tt
                elif self.state == 2 and v:
                    self.state = 1
                if self.state == 2 and not v and tt >= self.c + 2 * P:
                    ev.append((2, self.c + P)); self.state = 0
            self.fin = upto
        if fl & 2:
            if self.state:
                ev.append((2, self.m if self.state == 1 else min(self.c + P, self.m)))
            self.__init__()
        else:
            keep = min(len(self.x), 2 * h)
            self.x = self.x[len(self.x) - keep:]
        return ev


host = [HostSlot() for _ in range(B)]
pool = pools["with"]
host_ms, copy_ms, n_host_events, n_dev_events = [], [], 0, 0
for slot in host:                                                                         # the host walkers join mid-stream: time only
    slot.state = 0
for _ in range(args.host_steps):
    i = at["with"]
    step("with")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    probs, counts, fl = pool["probs"].cpu().numpy(), pool["counts"].cpu().numpy(), flags[i].cpu().numpy()
    t1 = time.perf_counter()
    for b in range(B):
        n_host_events += len(host[b].step(probs[b, :counts[b]], int(fl[b])))
    t2 = time.perf_counter()
    copy_ms.append((t1 - t0) * 1e3)
    host_ms.append((t2 - t0) * 1e3)
    n_dev_events += int(pool["endpoint"]["ev_counts"].sum())

base, withep = float(np.median(blocks["without"])), float(np.median(blocks["with"]))
res = {"config": f"{B} {'int16 PyanNet' if wav else 'f32 PyanNet2 (bidirectional, F 64)'} slots x {C}-sample chunks, W = {W}, L = {L}, endpoint kernel {K} "
                 f"pad {P}; {args.rounds} blocks of {args.steps} graph replays per setting, alternated, after a {warm}-step warm-up each",
       "step_ms_without": base, "step_ms_with": withep, "blocks_without": blocks["without"], "blocks_with": blocks["with"],
       "added_ms_per_step": withep - base, "added_fraction_of_step": (withep - base) / base,
       "host_alternative_ms_per_step": float(np.median(host_ms)), "host_copy_ms_per_step": float(np.median(copy_ms)),
       "host_over_added": float(np.median(host_ms)) / max(withep - base, 1e-6),
       "events_in_host_steps": {"device": n_dev_events, "host_walkers": n_host_events},
       "graphs": {k: v["graphs"] for k, v in pools.items()},
       "what": ("step_ms = HIP events around the replay of the pool's one graph, median of a block, then median over blocks; added = with - "
                "without; host alternative = wall time of copying the step's probabilities, counts and flags to the host plus 512 Python "
                "endpointers (the walkers join a running stream, so their event count only roughly matches the device's)")}
print(json.dumps(res))
