#!/usr/bin/env python3
"""What cutting a batch's speech out on the device costs (uvad_cuts_table + uvad_cuts_gather) against the host route it
replaces, at two shapes of int16 audio: 256 rows x 10 s (T = 1000) and one 1-hour row (T = 360000); pad 10, max_len 1000, min_len 10
frames, hop 160, tail 240; labels from the seeded x4 network on synthetic audio through the median filter (49 taps).
  (a) device  one captured graph of table + gather, replayed: nothing returns to the host;
  (b) host    labels_to_intervals_batch (one copy of the runs to the host) -> merge_intervals_with_buffer -> split_into_windows ->
              one slice of the device tensor per segment -> pad_sequence, ending in a synchronise.
The two alternate in blocks, --rounds times, in one process after --warmup calls of each.  (a): device events around --steps replays
of the graph, divided by --steps; (b): a host clock around --host-steps calls.  A block reports its mean per call; reported is the median
over blocks.  The gather alone is replayed the same way, and its bytes -- the samples read plus the whole padded batch written -- over
that time are set against the HBM rates of MI355X_MICROARCH.md.  --out writes the JSON (profiles/cuts.json)."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.postprocess import labels_to_intervals_batch, merge_intervals_with_buffer, split_into_windows
from uvad_amd.synth import seed_weights, synth_pcm_device

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="graph replays per block")
ap.add_argument("--host-steps", type=int, default=3, help="host-route calls per block")
ap.add_argument("--rounds", type=int, default=3, help="blocks of each route, alternated")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("run_cuts.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12       # bytes / s: spec, and the measured float4 copy (MI355X_MICROARCH.md)
P, W, M, HOP, TAIL, SHIFT = 10, 1000, 10, 160, 240, 0.01

m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=64); m.build(); seed_weights(m, 1234, 4.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=64, window_type="hamming"))
m = m.to(dev).eval()
rt = m.runtime(dev)


def network_labels(rows, seed):
    """rows x 10 s of seeded synthetic int16 audio -> (pcm (rows, 160000) int16, labels (rows, 1000) uint8), both on the device."""
    pcm = torch.round(synth_pcm_device(rows, 160000, seed=seed, device=dev) * 32767.0).to(torch.int16)
    probs = torch.cat([m.forward_waveform(pcm[i:i + 128])[1] for i in range(0, rows, 128)])
    return pcm, rt.median_filter(probs[:, :1000].contiguous(), 49)


def replay_ms(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def shape(pcm, labels):
    B, T = labels.shape
    S = pcm.shape[1]
    cfg = dict(pad=P, max_len=W, min_len=M, hop=HOP, lead=0, tail=TAIL)
    count = rt.cuts_open(**cfg)
    rt.cuts_table(labels, S=S, cuts=count)
    max_cuts = -(-max(len(rt.cuts_read(count)), 1) // 64) * 64      # the batch is max_cuts x ld_out samples: a bound near the total, as a caller would set
    ct = rt.cuts_open(max_cuts=max_cuts, **cfg)
    rt.speech_cuts(labels, pcm, cuts=ct)                    # sizes the buffers
    torch.cuda.synchronize()
    both, gather = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(both):
        table, batch, lens = rt.speech_cuts(labels, pcm, cuts=ct)
    with torch.cuda.graph(gather):
        rt.cuts_gather(pcm, ct, "samples")
    ld_out = batch.shape[1]

    def host_route():
        ivs = labels_to_intervals_batch(labels, SHIFT, runtime=rt)
        segs = []
        for b, iv in enumerate(ivs):
            for s, e in split_into_windows(merge_intervals_with_buffer(iv, T * SHIFT, P * SHIFT), W * SHIFT):
                segs.append(pcm[b, int(round(s * 16000)):min(int(round(e * 16000)) + TAIL, S)])
        out = torch.nn.utils.rnn.pad_sequence(segs, batch_first=True) if segs else pcm.new_zeros((0, 0))
        torch.cuda.synchronize()
        return out

    def host_ms(n):
        t0 = time.perf_counter()
        for _ in range(n):
            host_route()
        return (time.perf_counter() - t0) * 1e3 / n

    for _ in range(args.warmup):
        both.replay(); gather.replay()
    host_ms(1)
    torch.cuda.synchronize()
    blocks = {"device": [], "gather": [], "host": []}
    for _ in range(args.rounds):
        blocks["device"].append(replay_ms(both, args.steps))
        blocks["host"].append(host_ms(args.host_steps))
        blocks["gather"].append(replay_ms(gather, args.steps))
    tab = rt.cuts_read(ct)
    n = len(tab)
    n_host = int(host_route().shape[0])
    read_b = int(np.minimum(tab["n_samples"], ld_out).sum()) * 2 + n * 32
    write_b = n * ld_out * 2 + n * 4
    r = {"B": B, "T": T, "S": S, "cuts": n, "max_cuts": max_cuts, "host_route_segments": n_host, "ld_out": ld_out, "speech_frames": int(labels.sum().item()),
         "table_plus_gather_ms_per_replay": float(np.median(blocks["device"])), "gather_ms_per_replay": float(np.median(blocks["gather"])),
         "host_route_ms_per_call": float(np.median(blocks["host"])), "blocks_ms": blocks,
         "gather_bytes_read": read_b, "gather_bytes_written": write_b}
    r["table_ms_per_replay_by_difference"] = r["table_plus_gather_ms_per_replay"] - r["gather_ms_per_replay"]
    r["gather_bytes_per_s_over_replay_time"] = (read_b + write_b) / (r["gather_ms_per_replay"] * 1e-3)
    r["gather_share_of_hbm_copy_rate_6.29TBs"] = r["gather_bytes_per_s_over_replay_time"] / HBM_COPY
    r["gather_share_of_hbm_peak_8TBs"] = r["gather_bytes_per_s_over_replay_time"] / HBM_PEAK
    r["host_over_device"] = r["host_route_ms_per_call"] / r["table_plus_gather_ms_per_replay"]
    return r


pcm256, lab256 = network_labels(256, seed=1)
pcm360, lab360 = network_labels(360, seed=2)               # 360 x 10 s laid end to end: one 1-hour row
hour_pcm = torch.cat([pcm360.reshape(1, -1), pcm360.new_zeros((1, TAIL))], dim=1).contiguous()
out = {"pad": P, "max_len": W, "min_len": M, "hop": HOP, "tail": TAIL, "steps": args.steps, "host_steps": args.host_steps, "rounds": args.rounds,
       "timing": "device: HIP events around `steps` graph replays / steps; host: perf_counter around `host_steps` calls, each ending in a synchronise",
       "shapes": [shape(pcm256, lab256), shape(hour_pcm, lab360.reshape(1, -1).contiguous())]}
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
