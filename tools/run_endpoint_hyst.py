#!/usr/bin/env python3
"""What the two live endpointers cost per step, measured the same way in one run on one box: the hysteresis
endpointer (uvad_endpoint_hyst_step) and the median endpointer (uvad_endpoint_step, kernel 25), each
  alone     one captured graph holding the step alone, at 512 feeds and the ld_in a 20 ms slot pool step produces, on seeded
            block-structured probabilities: --frames new frames per feed and step (2 = what 20 ms of 10 ms frames gives; 0 = ld_in, a row
            as full as a flush makes it).  Blocks of --steps replays between one pair of HIP events, the endpointers alternated,
            --rounds blocks each; reported: the median over blocks of block time / replays;
  as a node the step behind the slot pool step in the pool's one graph (window_slots_open(..., endpoint=...)), sessions of seeded
            U(2, 30) s lengths starting and ending throughout as in tools/run_endpoint.py: three pools -- no endpointer, hysteresis, median
            -- alternated in blocks, every replay timed with HIP events, a block reports its median; added = with - without.
--no-pool skips the second part (no model is built).  One JSON line."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.runtime import VadRuntime, window_slots_ld_out
from uvad_amd.synth import seed_weights

ap = argparse.ArgumentParser()
ap.add_argument("--feeds", type=int, default=512)
ap.add_argument("--chunk", type=int, default=320)
ap.add_argument("--frames", type=int, default=2, help="new frames per feed and step of the stand-alone runs; 0 = ld_in")
ap.add_argument("--steps", type=int, default=400, help="replays per block")
ap.add_argument("--rounds", type=int, default=5, help="blocks of each setting, alternated")
ap.add_argument("--no-pool", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
B, C = args.feeds, args.chunk
W, L = 500, 50
HYST = {"onset": 0.6, "offset": 0.4, "min_on": 25, "min_off": 10, "pad_on": 10, "pad_off": 10}
MEDIAN = {"kernel": 25, "pad": 10}
ld_in = window_slots_ld_out(C, L, 160)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def alone(frames):
    """Per-replay time of each endpointer's step alone, in ms."""
    rt = VadRuntime(dev)
    rng = np.random.default_rng(3)
    p = np.empty((B, ld_in), np.float32)
    for b in range(B):                                                                    # speech / silence blocks of 1 .. 30 frames, MID inside
        t = 0
        while t < ld_in:
            n = int(rng.integers(1, 31))
            p[b, t:t + n] = (0.9, 0.5, 0.1)[int(rng.integers(0, 3))] + rng.uniform(-0.05, 0.05)
            t += n
    probs = torch.from_numpy(p).to(dev)
    counts = torch.full((B,), frames, dtype=torch.int32, device=dev)
    flags = torch.zeros(B, dtype=torch.uint8, device=dev)
    eps = {"hysteresis": (rt.endpoint_hyst_open(B, ld_in, **HYST), rt._endpoint_hyst_enqueue),
           "median": (rt.endpoint_open(B, ld_in, **MEDIAN), rt._endpoint_enqueue)}
    graphs = {}
    for name, (ep, enqueue) in eps.items():
        cur = torch.cuda.current_stream(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            r = enqueue(ep, probs.data_ptr(), counts.data_ptr(), flags.data_ptr())
        assert r == 0
        torch.cuda.current_stream(dev).wait_stream(cur)
        for _ in range(50):
            g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    blocks = {k: [] for k in graphs}
    for r in range(args.rounds):
        for name in (list(graphs) if r % 2 == 0 else list(graphs)[::-1]):
            e0.record()
            for _ in range(args.steps):
                graphs[name].replay()
            e1.record()
            torch.cuda.synchronize()
            blocks[name].append(e0.elapsed_time(e1) / args.steps)
    events = {k: int(eps[k][0]["ev_counts"].sum()) for k in eps}
    rt.close()
    return {k: {"ms_per_replay": float(np.median(v)), "blocks": v, "events_last_step": events[k]} for k, v in blocks.items()}


def as_node():
    m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=64); m.build(); seed_weights(m, 1234, 2.0)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=64))
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    g = torch.Generator(device=dev); g.manual_seed(5)
    audio = 0.1 * torch.randn(B, 64 * C, generator=g, device=dev)                         # 64 distinct chunks, cycled
    chunk_of = lambda i: audio[:, (i % 64) * C:(i % 64 + 1) * C].contiguous()
    warm = -(-(W * 160 + 400) // C)                                                       # steps until the window is full
    rng = np.random.default_rng(7)
    total = warm + args.steps * args.rounds + 80
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
    pools = {name: rt.window_slots_open(B, C, window=W, lookahead=L, graphs=True, endpoint=ep)
             for name, ep in (("without", None), ("hysteresis", HYST), ("median", MEDIAN))}
    assert pools["without"]["out"].shape[1] == ld_in
    at = dict.fromkeys(pools, 0)
    for name, pool in pools.items():                                                      # warm-up until every window is full
        for _ in range(warm):
            i = at[name]
            rt.window_slots_step(pool, chunk_of(i), start=flags[i] & 1 == 1, end=flags[i] & 2 == 2)
            at[name] = i + 1
    torch.cuda.synchronize()

    def replay_ms(name):
        """Device time of the graph replay alone (the chunk and flag copies in front of it are the same in every setting)."""
        pool, i = pools[name], at[name]
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
    for r in range(args.rounds):
        for name in order[r % 3:] + order[:r % 3]:
            blocks[name].append(float(np.median([replay_ms(name) for _ in range(args.steps)])))
    med = {k: float(np.median(v)) for k, v in blocks.items()}
    return {"step_ms": med, "blocks": blocks,
            "added_ms_per_step": {k: med[k] - med["without"] for k in ("hysteresis", "median")},
            "added_fraction_of_step": {k: (med[k] - med["without"]) / med["without"] for k in ("hysteresis", "median")},
            "spread_of_without_ms": float(max(blocks["without"]) - min(blocks["without"])),
            "graphs": {k: v["graphs"] for k, v in pools.items()}}


res = {"config": f"{B} feeds, ld_in {ld_in} (log-mel slot pool, {C}-sample chunks, W = {W}, L = {L}); hysteresis {HYST}; median {MEDIAN}; "
                 f"{args.rounds} blocks of {args.steps} graph replays per setting, alternated",
       "alone": {f"{args.frames or ld_in}_frames_per_step": alone(args.frames or ld_in), f"{ld_in}_frames_per_step": alone(ld_in)},
       "what": ("alone: HIP events around a block of back-to-back replays of a graph that holds the step alone, block time / replays, median "
                "over blocks; as a node: HIP events around each replay of the pool's one graph, median of a block, then median over blocks; "
                "added = with - without")}
if not args.no_pool:
    res["as_node"] = as_node()
print(json.dumps(res))
