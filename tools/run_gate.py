#!/usr/bin/env python3
"""What the live speech gate costs per step, measured as tools/run_endpoint_hyst.py measures the endpointers:
  alone     one captured graph holding uvad_gate_step alone, at 512 feeds of 320-sample f32 chunks, every feed inside a long speech run
            that splits every --max-len frames (2 new labels and one chunk per step: what 20 ms gives), blocks of --steps replays between
            one pair of HIP events, --rounds blocks; reported: the median over blocks of block time / replays;
  as a node the step behind the hysteresis endpointer behind the log-mel slot pool step, in the pool's one graph
            (window_slots_open(..., endpoint=..., gate=...)), sessions of seeded U(2, 30) s lengths starting and ending throughout, onset and
            offset put at percentiles of the probabilities the model emits so that about half of the frames are speech: two pools
            -- endpointer alone, endpointer + gate -- alternated in blocks, every replay timed with HIP events, a block reports its
            median; added = with - without, to be read against the spread between the blocks of the pool without the gate.
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
ap.add_argument("--max-len", type=int, default=1000, help="frames per piece (10 s at 10 ms frames)")
ap.add_argument("--steps", type=int, default=400, help="replays per block")
ap.add_argument("--rounds", type=int, default=5, help="blocks of each setting, alternated")
ap.add_argument("--no-pool", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
B, C = args.feeds, args.chunk
W, L = 500, 50
HYST = {"onset": 0.6, "offset": 0.4, "min_on": 25, "min_off": 10, "pad_on": 10, "pad_off": 10}
GATE = {"max_len": args.max_len}
ld_in = window_slots_ld_out(C, L, 160)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def alone():
    """Per-replay time of the gate's step alone, in ms: every feed delivers one chunk of speech audio per step."""
    rt = VadRuntime(dev)
    g = rt.gate_open(B, C, ld_in, torch.float32, L + 2, hop=160, lead=120, tail=120, **GATE)
    chunk = torch.randn(B, C, device=dev)
    labels = torch.ones((B, ld_in), dtype=torch.uint8, device=dev)
    counts = torch.full((B,), 2, dtype=torch.int32, device=dev)
    rt.gate_step(g, chunk, labels, torch.zeros_like(counts), start=torch.ones(B, dtype=torch.bool, device=dev))   # every session starts
    flags = torch.zeros(B, dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = rt._gate_enqueue(g, chunk.data_ptr(), labels.data_ptr(), counts.data_ptr(), flags.data_ptr())
    assert r == 0
    torch.cuda.current_stream(dev).wait_stream(cur)
    for _ in range(50):
        graph.replay()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(args.rounds):
        e0.record()
        for _ in range(args.steps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        blocks.append(e0.elapsed_time(e1) / args.steps)
    seg = g["seg"].cpu().numpy()
    res = {"ms_per_replay": float(np.median(blocks)), "blocks": blocks, "records_last_step": int(g["seg_counts"].sum()),
           "samples_last_step": int(seg[:, 0, 7].sum()), "state_bytes": int(g["state"].numel()), "history": g["history"],
           "ld_out": g["ld_out"], "max_seg": g["max_seg"]}
    rt.close()
    return res


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
    # onset / offset at the 45th / 25th percentile of what this model emits on this audio, so that about half of the frames are speech
    # and the gate has audio to deliver (seeded weights on noise sit on one side of any fixed threshold)
    probe, seen = rt.window_slots_open(B, C, window=W, lookahead=L, graphs=True), []
    for i in range(warm):
        lg, cnt = rt.window_slots_step(probe, chunk_of(i), start=flags[i] & 1 == 1, end=flags[i] & 2 == 2)
        if i >= warm - 20:
            seen.append(torch.cat([lg[b, :int(n)] for b, n in enumerate(cnt.tolist()) if n]))
    emitted = torch.cat(seen).double().cpu().numpy()
    sig = lambda z: float(np.float32(1.0 / (1.0 + np.exp(-z))))
    hyst = dict(HYST, onset=sig(np.percentile(emitted, 45)), offset=sig(np.percentile(emitted, 25)))
    del probe
    pools = {name: rt.window_slots_open(B, C, window=W, lookahead=L, graphs=True, endpoint=hyst, gate=gate)
             for name, gate in (("without", None), ("gate", GATE))}
    at = dict.fromkeys(pools, 0)
    records = samples = 0
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
        for name in order[r % 2:] + order[:r % 2]:
            blocks[name].append(float(np.median([replay_ms(name) for _ in range(args.steps)])))
            if name == "gate":                                                            # what the block's last step delivered
                gq = pools["gate"]["gate"]
                records += int(gq["seg_counts"].sum())
                samples += sum(int(frag.numel()) for *_, frag in rt.gate_collect(gq))
    med = {k: float(np.median(v)) for k, v in blocks.items()}
    gp = pools["gate"]["gate"]
    return {"step_ms": med, "blocks": blocks, "added_ms_per_step": med["gate"] - med["without"],
            "added_fraction_of_step": (med["gate"] - med["without"]) / med["without"],
            "spread_of_without_ms": float(max(blocks["without"]) - min(blocks["without"])),
            "endpoint": hyst, "records_in_sampled_steps": records, "samples_in_sampled_steps": samples, "gate": {k: gp[k] for k in ("history", "ld_lab", "ld_out", "max_seg", "lag_frames")},
            "gate_state_bytes": int(gp["state"].numel()), "graphs": {k: v["graphs"] for k, v in pools.items()}}


res = {"config": f"{B} feeds, {C}-sample f32 chunks, log-mel slot pool W = {W}, L = {L}, ld_in {ld_in}; hysteresis endpointer {HYST} with onset / offset replaced by percentiles of the emitted probabilities (as_node.endpoint); gate {GATE} "
                 f"with the pool's geometry; {args.rounds} blocks of {args.steps} graph replays per setting, alternated",
       "alone": alone(),
       "what": ("alone: HIP events around a block of back-to-back replays of a graph that holds the gate step alone, block time / replays, "
                "median over blocks; as a node: HIP events around each replay of the pool's one graph, median of a block, then median over "
                "blocks; added = with - without")}
if not args.no_pool:
    res["as_node"] = as_node()
print(json.dumps(res))
