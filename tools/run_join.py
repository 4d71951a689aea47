#!/usr/bin/env python3
"""What joining a batch's cuts with its supervisions costs on the device (uvad_cuts_join) against the host route it
replaces, at two shapes: 256 rows x 10 s (T = 1000) with about 8 supervisions per row, and one 1-hour row (T = 360000) with 2000
supervisions (overlap) and, separately, 10000 words (inside).  Cuts as tools/run_cuts.py: pad 10, max_len 1000, min_len 10 frames, hop
160, tail 240, labels from the seeded x4 network on synthetic audio through the median filter (49 taps); the items are seeded.
  (a) device  one captured graph of table + join, replayed; the join node alone; and table + gather + join, for the join's share;
  (b) host    cuts_read (one copy of the table to the host, which synchronises) plus a Python walk of cuts x items of each row that
              builds the same per-cut lists.
Device: HIP events around --steps replays, divided by --steps, the median over --rounds blocks, after --warmup replays.  Host: a host
clock around each call, the median over --host-calls calls (the 1-hour walks take seconds, so few).  The two routes' lists are compared
before anything is reported.  --out writes the JSON (profiles/join.json)."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.synth import seed_weights, synth_pcm_device

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="graph replays per block")
ap.add_argument("--rounds", type=int, default=3, help="blocks per graph")
ap.add_argument("--host-calls", type=int, default=3, help="host-route calls at the small shape (the 1-hour row: one per item list)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("run_join.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
P, W, M, HOP, TAIL = 10, 1000, 10, 160, 240

m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=64); m.build(); seed_weights(m, 1234, 4.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=64, window_type="hamming"))
m = m.to(dev).eval()
rt = m.runtime(dev)


def network_labels(rows, seed):
    pcm = torch.round(synth_pcm_device(rows, 160000, seed=seed, device=dev) * 32767.0).to(torch.int16)
    probs = torch.cat([m.forward_waveform(pcm[i:i + 128])[1] for i in range(0, rows, 128)])
    return pcm, rt.median_filter(probs[:, :1000].contiguous(), 49)


def seeded_items(rng, B, T, per_row, lo, hi):
    """(B, per_row, 2) int32 frames: starts uniform over the row, sorted, lengths uniform in [lo, hi]; counts vary a little per row."""
    s = np.sort(rng.integers(0, T, (B, per_row)), axis=1)
    iv = np.stack([s, s + rng.integers(lo, hi + 1, (B, per_row))], axis=2).astype(np.int32)
    counts = rng.integers(max(per_row - 3, 0), per_row + 1, B).astype(np.int32) if B > 1 else np.asarray([per_row], np.int32)
    return iv, counts


def replay_ms(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def host_walk(tab, iv, counts, inside):
    """The loop a user writes today: for every cut, every item of its row."""
    out = []
    for c in tab:
        b, f, e = int(c["row"]), int(c["first_frame"]), int(c["first_frame"]) + int(c["n_frames"])
        mine = []
        for j in range(int(counts[b])):
            s, t = int(iv[b, j, 0]), int(iv[b, j, 1])
            if t > s and ((s >= f and t <= e) if inside else (s < e and t > f)):
                mine.append(j)
        out.append(mine)
    return out


def shape(name, pcm, labels, iv, counts, mode, host_calls):
    B, T = labels.shape
    S = pcm.shape[1]
    cfg = dict(pad=P, max_len=W, min_len=M, hop=HOP, lead=0, tail=TAIL)
    count = rt.cuts_open(**cfg)
    rt.cuts_table(labels, S=S, cuts=count)
    max_cuts = -(-max(len(rt.cuts_read(count)), 1) // 64) * 64          # a bound near the total, as a caller would set
    ct = rt.cuts_open(max_cuts=max_cuts, **cfg)
    d_iv, d_cnt = torch.from_numpy(iv).to(dev), torch.from_numpy(counts).to(dev)
    max_pairs = max_cuts + 4 * int(counts.sum())                        # the seeded items overlap one another: room for four cuts an item
    rt.speech_cuts(labels, pcm, cuts=ct)                                # sizes the buffers
    rt.cuts_join(ct, d_iv, d_cnt, mode=mode, max_pairs=max_pairs)
    torch.cuda.synchronize()
    graphs = {k: torch.cuda.CUDAGraph() for k in ("table_join", "join", "table_gather_join", "table_gather")}
    with torch.cuda.graph(graphs["table_join"]):
        rt.cuts_table(labels, S=S, cuts=ct)
        rt.cuts_join(ct, d_iv, d_cnt, mode=mode, max_pairs=max_pairs)
    with torch.cuda.graph(graphs["join"]):
        rt.cuts_join(ct, d_iv, d_cnt, mode=mode, max_pairs=max_pairs)
    with torch.cuda.graph(graphs["table_gather_join"]):
        rt.speech_cuts(labels, pcm, cuts=ct)
        rt.cuts_join(ct, d_iv, d_cnt, mode=mode, max_pairs=max_pairs)
    with torch.cuda.graph(graphs["table_gather"]):
        rt.speech_cuts(labels, pcm, cuts=ct)
    for _ in range(args.warmup):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    blocks = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            blocks[k].append(replay_ms(g, args.steps))
    graphs["table_join"].replay()
    read = rt.cuts_join_read(ct)

    def host_route():
        t0 = time.perf_counter()
        lists = host_walk(rt.cuts_read(ct), iv, counts, mode == "inside")
        return (time.perf_counter() - t0) * 1e3, lists

    host = [host_route() for _ in range(host_calls)]
    assert all(lists == read["pairs_per_cut"] for _, lists in host), "the two routes disagree"
    med = {k: float(np.median(v)) for k, v in blocks.items()}
    r = {"shape": name, "mode": mode, "B": B, "T": T, "items": int(counts.sum()), "max_iv": int(iv.shape[1]), "cuts": len(read["pairs_per_cut"]),
         "max_cuts": max_cuts, "pairs": read["total_pairs"], "audit": read["audit"]["pooled"],
         "table_plus_join_ms_per_replay": med["table_join"], "join_ms_per_replay": med["join"],
         "table_plus_gather_plus_join_ms_per_replay": med["table_gather_join"], "table_plus_gather_ms_per_replay": med["table_gather"],
         "host_route_ms_per_call": float(np.median([t for t, _ in host])), "host_calls": host_calls, "blocks_ms": blocks}
    r["host_over_table_plus_join"] = r["host_route_ms_per_call"] / r["table_plus_join_ms_per_replay"]
    r["join_share_of_table_gather_join"] = r["join_ms_per_replay"] / r["table_plus_gather_plus_join_ms_per_replay"]
    return r


rng = np.random.default_rng(2024)
pcm256, lab256 = network_labels(256, seed=1)
pcm360, lab360 = network_labels(360, seed=2)               # 360 x 10 s laid end to end: one 1-hour row
hour_pcm = torch.cat([pcm360.reshape(1, -1), pcm360.new_zeros((1, TAIL))], dim=1).contiguous()
hour_lab = lab360.reshape(1, -1).contiguous()
out = {"pad": P, "max_len": W, "min_len": M, "hop": HOP, "tail": TAIL, "steps": args.steps, "rounds": args.rounds,
       "timing": "device: HIP events around `steps` graph replays / steps, median over `rounds` blocks; host: perf_counter around cuts_read + a Python "
                 "walk of cuts x items, median over `host_calls` calls",
       "shapes": [shape("256 x 1000 frames, about 8 supervisions of 0.5-2 s per row", pcm256, lab256, *seeded_items(rng, 256, 1000, 8, 50, 200), "overlap", args.host_calls),
                  shape("1 x 360000 frames, 2000 supervisions of 1-3 s", hour_pcm, hour_lab, *seeded_items(rng, 1, 360000, 2000, 100, 300), "overlap", 1),
                  shape("1 x 360000 frames, 10000 words of 0.1-0.5 s", hour_pcm, hour_lab, *seeded_items(rng, 1, 360000, 10000, 10, 50), "inside", 1)]}
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
