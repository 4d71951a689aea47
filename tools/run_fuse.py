#!/usr/bin/env python3
"""What fusing the channels of a batch costs on the device (uvad_fuse, uvad_fuse_pick) against the torch route it
replaces, at four shapes: 256 recordings x 2 channels x 1000 frames, 32 x 8 channels x 1000 frames, one 1-hour row of 8 channels
(T = 360000), and the node behind a 512-feed slot pool step (256 two-channel groups, T = the pool's ld_out for 100 ms chunks, counts as a
step gives them).  Probabilities are seeded random walks clipped to [0, 1]: the cost does not depend on the values.
  (a) device  one captured graph of uvad_fuse (labels, best and the counters on), replayed; and, at the three offline shapes, one graph of
              fuse + uvad_cuts_table + uvad_fuse_pick + uvad_cuts_gather of int16 audio (pad 10, max_len 1000, min_len 10, hop 160,
              tail 240);
  (b) torch   index_select of the members + max (or the mean) + argmax + the four counts + .cpu() of the counts, on the same GPU: what
              a caller writes today, ending in the copy the device route does not need.
Device: HIP events around --steps replays, divided by --steps, the median over --rounds blocks, after --warmup replays.  Torch: a host
clock around each call (it ends in a synchronising copy), the median over --host-calls calls.  The two routes' fused rows are compared
before anything is reported.  Effective bytes/s of the fuse node = frames x (4 M + 6) bytes / time, set against the float4 copy rate
profiles/cuts.json records (6.29 TB/s).  --out writes the JSON (profiles/fuse.json)."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd  # noqa: F401
from uvad_amd.runtime import VadRuntime, window_slots_ld_out

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="graph replays per block")
ap.add_argument("--rounds", type=int, default=3, help="blocks per graph")
ap.add_argument("--host-calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("run_fuse.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
COPY_RATE = 6.29e12
rt = VadRuntime(dev)
CUTS = dict(pad=10, max_len=1000, min_len=10, hop=160, lead=0, tail=240)


def replay_ms(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def blocks_of(graph):
    for _ in range(args.warmup):
        graph.replay()
    torch.cuda.synchronize()
    return [replay_ms(graph, args.steps) for _ in range(args.rounds)]


def torch_route(x, idx, lens_g, mode, thr):
    """x (B, T); idx (G, M) member rows; dense members of equal length per group (what the route can do without a loop)."""
    G, M = idx.shape
    v = x.index_select(0, idx.reshape(-1)).reshape(G, M, -1)
    fused = v.max(dim=1).values if mode == "max" else v.mean(dim=1, dtype=torch.float64).to(torch.float32)
    best = v.argmax(dim=1)
    lab = ~(fused < thr)
    own = ~(v < thr)
    valid = (torch.arange(v.shape[2], device=x.device)[None, None, :] < lens_g[:, None, None]).expand_as(own)
    counts = torch.stack([valid.sum(2), (own & valid).sum(2), ((own == lab[:, None, :]) & valid).sum(2),
                          ((best[:, None, :] == torch.arange(M, device=x.device)[None, :, None]) & valid).sum(2)], dim=2)
    return fused, best, counts.cpu()


def shape(name, G, M, T, mode, with_cuts, lens=None, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    B = G * M
    x = (0.5 + torch.cumsum(torch.randn((B, T), device=dev, generator=g) * 0.05, dim=1)).clamp_(0, 1).contiguous()
    groups = [[r * M + c for c in range(M)] for r in range(G)]
    d_lens = None if lens is None else torch.from_numpy(np.repeat(lens, M).astype(np.int32)).to(dev)
    st = rt.fuse_open(groups, mode=mode, threshold=0.5)
    fused, glens, labels, best, stats = rt.fuse(x, lengths=d_lens, state=st)           # sizes the buffers
    torch.cuda.synchronize()
    graphs = {"fuse": torch.cuda.CUDAGraph()}
    with torch.cuda.graph(graphs["fuse"]):
        rt.fuse(x, lengths=d_lens, state=st)
    r = {"shape": name, "mode": mode, "groups": G, "members": M, "T": T}
    if with_cuts:
        S = T * CUTS["hop"] + CUTS["tail"]
        pcm = torch.randint(-32768, 32767, (B, S), dtype=torch.int16, device=dev, generator=g)
        count = rt.cuts_open(**CUTS)
        rt.cuts_table(labels, lengths=glens, S=S, cuts=count)
        max_cuts = -(-max(len(rt.cuts_read(count)), 1) // 64) * 64                       # a bound near the total, as a caller would set
        ct = rt.cuts_open(max_cuts=max_cuts, **CUTS)
        rt.cuts_table(labels, lengths=glens, S=S, cuts=ct)
        ptab, _ = rt.fuse_pick(best, ct)
        rt.cuts_gather(pcm, ct, "samples", table=ptab)
        torch.cuda.synchronize()
        graphs["fuse_table_pick_gather"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs["fuse_table_pick_gather"]):
            _, gl, lab, bst, _ = rt.fuse(x, lengths=d_lens, state=st)
            rt.cuts_table(lab, lengths=gl, S=S, cuts=ct)
            pt, _ = rt.fuse_pick(bst, ct)
            rt.cuts_gather(pcm, ct, "samples", table=pt)
        r["cuts"], r["max_cuts"] = len(rt.cuts_read(ct)), max_cuts
    blocks = {k: blocks_of(gr) for k, gr in graphs.items()}
    idx = torch.tensor(groups, device=dev)
    lens_g = torch.full((G,), T, device=dev) if lens is None else torch.from_numpy(lens.astype(np.int64)).to(dev)
    host = []
    for _ in range(args.host_calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tf, tb, tc = torch_route(x, idx, lens_g, mode, 0.5)
        host.append((time.perf_counter() - t0) * 1e3)
    rt.fuse_reset_stats(st)
    graphs["fuse"].replay()
    torch.cuda.synchronize()
    gl = glens.cpu().tolist()
    for k in range(G):
        assert torch.equal(fused[k, :gl[k]], tf[k, :gl[k]]) or mode != "max", "the two routes disagree"
    assert stats.cpu()[:, 0].reshape(G, M).tolist() == tc[:, :, 0].tolist(), "the two routes disagree on the valid frames"
    frames = int(sum(gl))
    ms = float(np.median(blocks["fuse"]))
    r.update(frames=frames, fuse_ms_per_replay=ms, blocks_ms=blocks, torch_route_ms_per_call=float(np.median(host)), host_calls=args.host_calls,
             torch_over_fuse=float(np.median(host)) / ms, effective_bytes_per_s=frames * (4 * M + 6) / (ms * 1e-3),
             share_of_hbm_copy_rate_6_29TBs=frames * (4 * M + 6) / (ms * 1e-3) / COPY_RATE)
    if with_cuts:
        r["fuse_table_pick_gather_ms_per_replay"] = float(np.median(blocks["fuse_table_pick_gather"]))
    return r


ld = window_slots_ld_out(1600, 0)
rng = np.random.default_rng(2024)
out = {"cuts": CUTS, "steps": args.steps, "rounds": args.rounds,
       "timing": "device: HIP events around `steps` graph replays / steps, median over `rounds` blocks; torch: perf_counter around index_select + "
                 "reduce + argmax + counts + .cpu(), median over `host_calls` calls",
       "shapes": [shape("256 recordings x 2 channels x 1000 frames", 256, 2, 1000, "max", True, seed=1),
                  shape("32 recordings x 8 channels x 1000 frames", 32, 8, 1000, "mean", True, seed=2),
                  shape("1 recording x 8 channels x 360000 frames", 1, 8, 360000, "max", True, seed=3),
                  shape(f"behind a 512-feed pool step: 256 groups x 2 feeds x ld_out {ld}", 256, 2, ld, "max", False,
                        lens=rng.integers(0, ld + 1, 256), seed=4)]}
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
