#!/usr/bin/env python3
"""What the hysteresis decisions cost on the device (uvad_binarize) at two shapes of probabilities from the seeded x4
network on synthetic audio: 256 rows x 1000 frames and one 1-hour row of 360000; onset 0.6, offset 0.4, min_on 25, min_off 10, pad_on 3,
pad_off 6 frames (0.25 s, 0.1 s, 30 ms, 60 ms at 10 ms frames).
  (a) binarize  one captured graph of uvad_binarize with labels, replayed; and the same without labels (classify + rows kernels alone);
  (b) median    the device chain that was the only one before: uvad_median_filter_lens (49 taps) + uvad_label_runs_lens, plus
                uvad_cuts_table (pad 6, max_len 0) for the padded, merged intervals -- it computes something else; it is the neighbour
                to compare a cost with, not a result;
  (c) host      the route (a) replaces: the probabilities copied to the host and postprocess.hysteresis_runs on every row.
(a) and (b) alternate in blocks with (c), --rounds times, in one process after --warmup calls of each.  Device: HIP events around --steps
replays of a graph, divided by --steps; host: a host clock around --host-steps calls.  A block reports its mean per call; reported is the
median over blocks.  The classify kernel's 4 bytes per frame over the no-labels replay time is a LOWER bound of its rate (the replay
also holds the rows kernel); kernel times proper come from a kernel trace of --trace-only, which only replays (a).  --out writes the
JSON (profiles/binarize.json)."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.postprocess import hysteresis_runs
from uvad_amd.synth import seed_weights, synth_pcm_device

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="graph replays per block")
ap.add_argument("--host-steps", type=int, default=3, help="host-route calls per block")
ap.add_argument("--rounds", type=int, default=3, help="blocks of each route, alternated")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--trace-only", action="store_true", help="replay the binarize graphs --steps times each and stop (for a kernel trace)")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("run_binarize.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
HBM_COPY = 6.29e12                         # bytes / s: the measured float4 copy (MI355X_MICROARCH.md, README)
CFG = dict(onset=0.6, offset=0.4, min_on=25, min_off=10, pad_on=3, pad_off=6)
SPAN = 4096                                # frames per pass of binarize_rows_kernel

m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=64); m.build(); seed_weights(m, 1234, 4.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=64, window_type="hamming"))
m = m.to(dev).eval()
rt = m.runtime(dev)


def network_probs(rows, seed):
    """rows x 10 s of seeded synthetic int16 audio -> probabilities (rows, 1000) f32 on the device."""
    pcm = torch.round(synth_pcm_device(rows, 160000, seed=seed, device=dev) * 32767.0).to(torch.int16)
    return torch.cat([m.forward_waveform(pcm[i:i + 128])[1] for i in range(0, rows, 128)])[:, :1000].contiguous()


def replay_ms(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def shape(probs):
    B, T = probs.shape
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    st, st_nolab = rt.binarize_open(**CFG), rt.binarize_open(**CFG)
    rt.binarize(probs, lengths=lens, state=st)                      # sizes the buffers
    rt.binarize(probs, lengths=lens, state=st_nolab, labels=False)
    ct = rt.cuts_open(pad=CFG["pad_off"], max_len=0, min_len=0)
    rt.cuts_table(rt.median_filter(probs, 49, lengths=lens), lengths=lens, cuts=ct)
    torch.cuda.synchronize()
    g_bin, g_nolab, g_med, g_med_cuts = (torch.cuda.CUDAGraph() for _ in range(4))
    with torch.cuda.graph(g_bin):
        rt.binarize(probs, lengths=lens, state=st)
    with torch.cuda.graph(g_nolab):
        rt.binarize(probs, lengths=lens, state=st_nolab, labels=False)
    if args.trace_only:
        for g in (g_bin, g_nolab):
            replay_ms(g, args.steps)
        return {"B": B, "T": T}
    with torch.cuda.graph(g_med):
        lab = rt.median_filter(probs, 49, lengths=lens)
        runs, counts = rt.label_runs(lab, lengths=lens)
    with torch.cuda.graph(g_med_cuts):
        lab2 = rt.median_filter(probs, 49, lengths=lens)
        rt.label_runs(lab2, lengths=lens)
        rt.cuts_table(lab2, lengths=lens, cuts=ct)

    def host_route():
        p = probs.cpu().numpy()                                    # synchronises
        return [hysteresis_runs(p[b], CFG) for b in range(B)]

    def host_ms(n):
        t0 = time.perf_counter()
        for _ in range(n):
            host_route()
        return (time.perf_counter() - t0) * 1e3 / n

    graphs = {"binarize": g_bin, "binarize_no_labels": g_nolab, "median_runs": g_med, "median_runs_cuts": g_med_cuts}
    for _ in range(args.warmup):
        for g in graphs.values():
            g.replay()
    host_ms(1)
    torch.cuda.synchronize()
    blocks = {k: [] for k in list(graphs) + ["host"]}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            blocks[k].append(replay_ms(g, args.steps))
        blocks["host"].append(host_ms(args.host_steps))
    got = rt.binarize_read(st)
    if got != host_route():
        raise SystemExit("the device's intervals differ from the host walk's")
    med = {k: float(np.median(v)) for k, v in blocks.items()}
    passes = B * -(-T // SPAN)
    r = {"B": B, "T": T, "intervals": sum(len(x) for x in got), "speech_frames": int(st["labels"].sum().item()),
         "median_chain_runs": int(counts.sum().item()),
         "binarize_ms_per_replay": med["binarize"], "binarize_no_labels_ms_per_replay": med["binarize_no_labels"],
         "labels_ms_per_replay_by_difference": med["binarize"] - med["binarize_no_labels"],
         "median_runs_ms_per_replay": med["median_runs"], "median_runs_cuts_ms_per_replay": med["median_runs_cuts"],
         "host_walk_ms_per_call": med["host"], "blocks_ms": blocks,
         "probability_bytes": B * T * 4, "row_passes_of_4096_frames": passes,
         "classify_bytes_per_s_lower_bound_over_no_labels_replay": B * T * 4 / (med["binarize_no_labels"] * 1e-3),
         "no_labels_ms_per_serial_pass_upper_bound": med["binarize_no_labels"] / -(-T // SPAN)}
    r["classify_lower_bound_share_of_hbm_copy_rate_6.29TBs"] = r["classify_bytes_per_s_lower_bound_over_no_labels_replay"] / HBM_COPY
    r["host_over_device"] = med["host"] / med["binarize"]
    r["binarize_over_median_runs_cuts"] = med["binarize"] / med["median_runs_cuts"]
    return r


p256 = network_probs(256, seed=1)
hour = network_probs(360, seed=2).reshape(1, -1).contiguous()      # 360 x 10 s laid end to end: one 1-hour row
out = {**CFG, "steps": args.steps, "host_steps": args.host_steps, "rounds": args.rounds,
       "timing": "device: HIP events around `steps` graph replays / steps; host: perf_counter around `host_steps` calls, each starting with the copy of the probabilities",
       "shapes": [shape(p256), shape(hour)]}
print(json.dumps(out))
if args.out and not args.trace_only:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
