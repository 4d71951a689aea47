#!/usr/bin/env python3
"""Variable-length batches (uvad_forward_lens): N whole recordings of lengths uniform in [--min-seconds, --max-seconds], 16-bit PCM, a
bidirectional PyanNet2 (80-bin log-mel, the reference's defaults), run three ways on one GPU:
  (a) today's whole-recording path: one dense uvad_forward_i16 per distinct length (here every recording, B = 1 each);
  (b) ragged batches: recordings sorted by length and packed so that rows x the batch's longest row stay within --max-duration
      (predict_vad's pack_ragged_batches), one uvad_forward_lens_i16 per batch;
  (c) ONE dense call padded to the longest row -- a cost reference only: for a bidirectional model its answers are wrong.
Reports valid frames/s (sum over recordings of uvad_num_frames(S_b) / wall time of the whole set, each way timed after a warm-up pass)
and checks that (b) gives every recording the probabilities of (a) (max |difference|).  One JSON line."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.scripts import pack_ragged_batches
from uvad_amd.synth import seed_weights

ap = argparse.ArgumentParser()
ap.add_argument("--recordings", type=int, default=256)
ap.add_argument("--min-seconds", type=float, default=10.0)
ap.add_argument("--max-seconds", type=float, default=120.0)
ap.add_argument("--max-duration", type=float, default=4000.0, help="padded seconds of audio per ragged batch")
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--skip-padded", action="store_true", help="leave out (c)")
args = ap.parse_args()
dev = torch.device("cuda:0")
F, sr = 80, 16000
m = uvad_amd.PyanNet2(encoding_dim=F); m.build(); seed_weights(m, 1234, 2.0)
m.attach_fbank(uvad_amd.FbankConfig(num_filters=F)); m = m.to(dev).eval()
rt = m.runtime(dev)
rng = np.random.default_rng(7)
nsamp = [int(v) for v in rng.uniform(args.min_seconds * sr, args.max_seconds * sr, args.recordings)]
S = max(nsamp)
pcm = torch.from_numpy(np.round(rng.standard_normal((args.recordings, S)) * 3000).clip(-32768, 32767).astype(np.int16)).to(dev)
frames = [rt.num_frames(n) for n in nsamp]
valid = sum(frames)
batches = pack_ragged_batches(nsamp, int(args.max_duration * sr))
ragged_in = []
for grp in batches:   # inputs staged once, outside the timing: rows zero-padded to the batch's longest
    n = max(nsamp[i] for i in grp)
    ragged_in.append((grp, pcm[grp, :n].contiguous(), torch.tensor([nsamp[i] for i in grp], dtype=torch.int64, device=dev)))
dense_in = [pcm[i:i + 1, :nsamp[i]].contiguous() for i in range(args.recordings)]


def run_dense():
    return [rt.forward(x, want_logits=False)[1] for x in dense_in]


def run_ragged():
    return [(grp, rt.forward(x, want_logits=False, lengths=n)[1]) for grp, x, n in ragged_in]


def run_padded():
    return rt.forward(pcm, want_logits=False)[1]


def timed(fn):
    fn()                                   # warm-up: workspace, kernel attributes
    torch.cuda.synchronize()
    best = None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


dense, t_a = timed(run_dense)
ragged, t_b = timed(run_ragged)
err = 0.0
for grp, probs in ragged:
    for r, i in enumerate(grp):
        err = max(err, float((probs[r, :frames[i]] - dense[i][0]).abs().max()))
        assert torch.count_nonzero(probs[r, frames[i]:]) == 0
out = {"workload": f"{args.recordings} recordings x U({args.min_seconds:g}, {args.max_seconds:g}) s, int16 PCM, 80-bin log-mel + bidirectional "
                   f"PyanNet2 (4 x 128), one GPU",
       "valid_frames": valid, "audio_seconds": round(sum(nsamp) / sr, 1),
       "a_dense_per_length": {"calls": len(dense_in), "s": round(t_a, 4), "valid_frames_per_s": round(valid / t_a)},
       "b_ragged": {"calls": len(batches), "max_duration_s": args.max_duration, "rows_per_call": [len(g) for g in batches],
                    "s": round(t_b, 4), "valid_frames_per_s": round(valid / t_b), "time_chunks": rt.time_chunks(),
                    "max_abs_prob_diff_vs_a": err},
       "speedup_b_over_a": round(t_a / t_b, 2)}
del dense
if not args.skip_padded:
    _, t_c = timed(run_padded)
    out["c_padded_dense_reference"] = {"calls": 1, "padded_frames": args.recordings * rt.num_frames(S), "s": round(t_c, 4),
                                       "valid_frames_per_s": round(valid / t_c), "note": "wrong answers for a bidirectional model"}
# The recurrence follows each workgroup's longest row, not T: one classify at (B, T) = (64, 3000), time chunks off, timed with the library's
# events (uvad_set_timing), dense and with lengths (all T; all T / 4; T / 4 except one row of T in the first tile of four; every tile of
# four holding one row of T)
Bq, Tq = min(64, args.recordings), 3000
feats = rt.fbank(pcm[:Bq, :Tq * 160].to(torch.float32) / 32768.0)[:, :Tq].contiguous()
rt.set_time_chunks(1); rt.set_recurrent_tile(4); rt.set_timing(True)
cases = {"dense": None, "lens_all_T": [Tq] * Bq, "lens_all_T/4": [Tq // 4] * Bq,
         "lens_T/4_one_tile_T": [Tq] + [Tq // 4] * (Bq - 1), "lens_one_T_per_tile": [Tq if b % 4 == 0 else Tq // 4 for b in range(Bq)]}
rec = {}
for name, lens in cases.items():
    ms = []
    for _ in range(4):
        rt.classify(feats, want_probs=False, lengths=lens)
        torch.cuda.synchronize()
        ms.append(sum(r for _, r in rt.layer_timing_ms()))
    rec[name] = round(float(np.median(ms[1:])), 3)
rt.set_timing(False); rt.set_time_chunks(0); rt.set_recurrent_tile(0)
out[f"recurrence_ms_4_layers_B{Bq}_T{Tq}_tile4"] = rec
print(json.dumps(out))
