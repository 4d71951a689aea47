#!/usr/bin/env python3
"""What the group gate costs per step, measured as tools/run_gate.py measures the mono gate as a node: the 512-feed
log-mel slot pool (W 500, L 50, 320-sample f32 chunks) opened as 256 two-channel groups (fuse, mode max) with the hysteresis endpointer of
profiles/gate.json over the groups; sessions of seeded U(2, 30) s lengths start and end per group throughout; onset and offset sit at
percentiles of the probabilities the model emits, so that about half of the frames are speech.  Two pools -- fusion + endpointer, and
fusion + endpointer + group gate (--decide frames, --max-len) -- are alternated in blocks; every replay of a pool's one graph is timed
with HIP events, a block reports its median; added = with - without, to be read against the spread between the blocks of the pool without
the node ("not resolved" if it is below it).  One JSON line."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.synth import seed_weights

ap = argparse.ArgumentParser()
ap.add_argument("--feeds", type=int, default=512)
ap.add_argument("--chunk", type=int, default=320)
ap.add_argument("--decide", type=int, default=25, help="decide_frames (0.25 s at 10 ms frames)")
ap.add_argument("--max-len", type=int, default=1000, help="frames per piece (10 s at 10 ms frames)")
ap.add_argument("--steps", type=int, default=400, help="replays per block")
ap.add_argument("--rounds", type=int, default=5, help="blocks of each setting, alternated")
args = ap.parse_args()
dev = torch.device("cuda:0")
B, C = args.feeds, args.chunk
G = B // 2
W, L = 500, 50
HYST = {"onset": 0.6, "offset": 0.4, "min_on": 25, "min_off": 10, "pad_on": 10, "pad_off": 10}
GATE = {"decide_frames": args.decide, "max_len": args.max_len}
GROUPS = [[2 * g, 2 * g + 1] for g in range(G)]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=64); m.build(); seed_weights(m, 1234, 2.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=64))
m = m.to(dev).eval()
rt = m.runtime(dev)
g = torch.Generator(device=dev); g.manual_seed(5)
audio = 0.1 * torch.randn(B, 64 * C, generator=g, device=dev)                             # 64 distinct chunks, cycled; the channels differ
chunk_of = lambda i: audio[:, (i % 64) * C:(i % 64 + 1) * C].contiguous()
warm = -(-(W * 160 + 400) // C)                                                           # steps until the window is full
rng = np.random.default_rng(7)
total = warm + args.steps * args.rounds + 80
starts, ends = np.zeros((total, B), bool), np.zeros((total, B), bool)
for grp in GROUPS:                                                                        # the members of a group start and end together
    s = 0
    while s < total:
        n = int(rng.uniform(2, 30) * 16000 / C)
        starts[s, grp] = True
        if s + n - 1 < total:
            ends[s + n - 1, grp] = True
        s += n + int(rng.integers(0, 20))
flags = torch.from_numpy(starts.astype(np.uint8) | (ends.astype(np.uint8) << 1)).to(dev)
probe, seen = rt.window_slots_open(B, C, window=W, lookahead=L, graphs=True), []
for i in range(warm):
    lg, cnt = rt.window_slots_step(probe, chunk_of(i), start=flags[i] & 1 == 1, end=flags[i] & 2 == 2)
    if i >= warm - 20:
        seen.append(torch.cat([lg[b, :int(n)] for b, n in enumerate(cnt.tolist()) if n]))
emitted = torch.cat(seen).double().cpu().numpy()
sig = lambda z: float(np.float32(1.0 / (1.0 + np.exp(-z))))
# the fused value is the larger of two channels: its percentiles sit above a single channel's, so the thresholds go a little higher
hyst = dict(HYST, onset=sig(np.percentile(emitted, 70)), offset=sig(np.percentile(emitted, 50)))
del probe
pools = {name: rt.window_slots_open(B, C, window=W, lookahead=L, graphs=True, fuse={"groups": GROUPS, "mode": "max", "threshold": hyst["onset"]},
                                    endpoint=hyst, group_gate=gate)
         for name, gate in (("without", None), ("group_gate", GATE))}
at = dict.fromkeys(pools, 0)
for name, pool in pools.items():                                                          # warm-up until every window is full
    for _ in range(warm):
        i = at[name]
        rt.window_slots_step(pool, chunk_of(i), start=flags[i] & 1 == 1, end=flags[i] & 2 == 2)
        at[name] = i + 1
torch.cuda.synchronize()


def replay_ms(name):
    """Device time of the graph replay alone (the chunk and flag copies in front of it are the same in every setting)."""
    pool, i = pools[name], at[name]
    if rt._fuse_current is not pool["fuse"]:                                              # the context holds one fusion configuration
        rt._fuse_configure(pool["fuse"])
    pool["in"].copy_(chunk_of(i))
    pool["flags"].copy_(flags[i])
    torch.cuda.synchronize()
    e0.record()
    pool["graph"].replay()
    e1.record()
    torch.cuda.synchronize()
    at[name] = i + 1
    return e0.elapsed_time(e1)


blocks = {k: [] for k in pools}
order = list(pools)
records = samples = unsync = 0
channels = [0, 0]
for r in range(args.rounds):
    for name in order[r % 2:] + order[:r % 2]:
        blocks[name].append(float(np.median([replay_ms(name) for _ in range(args.steps)])))
        if name == "group_gate":                                                          # what the block's last step delivered
            for recs in rt.gate_group_collect(pools[name]["group_gate"]):
                for d in recs:
                    records += 1
                    samples += int(d["fragment"].numel())
                    channels[d["channel"]] += 1
                    unsync += bool(d["flags"] & 16)
med = {k: float(np.median(v)) for k, v in blocks.items()}
gp = pools["group_gate"]["group_gate"]
spread = float(max(blocks["without"]) - min(blocks["without"]))
added = med["group_gate"] - med["without"]
print(json.dumps({
    "config": f"{B} feeds as {G} two-channel groups, {C}-sample f32 chunks, log-mel slot pool W = {W}, L = {L}; fusion mode max; hysteresis "
              f"endpointer {HYST} with onset / offset replaced by percentiles of the emitted probabilities (endpoint); group gate {GATE} with the "
              f"pool's geometry; {args.rounds} blocks of {args.steps} graph replays per setting, alternated",
    "step_ms": med, "blocks": blocks, "added_ms_per_step": added, "added_fraction_of_step": added / med["without"],
    "spread_of_without_ms": spread, "resolved": bool(abs(added) > spread), "endpoint": hyst,
    "records_in_sampled_steps": records, "samples_in_sampled_steps": samples, "channels_in_sampled_steps": channels, "unsync_records": unsync,
    "group_gate": {k: gp[k] for k in ("history", "best_history", "decide_frames", "ld_lab", "ld_out", "max_seg", "lag_frames")},
    "group_gate_state_bytes": int(gp["state"].numel()), "graphs": {k: v["graphs"] for k, v in pools.items()},
    "what": "HIP events around each replay of the pool's one graph, median of a block, then median over blocks; added = with - without"}))
