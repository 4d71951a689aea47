#!/usr/bin/env python3
"""Variable-length batches of the waveform model (uvad_forward_wav_lens_i16): N whole recordings of lengths uniform in [--min-seconds,
--max-seconds], 16-bit PCM, the bidirectional 4 x 128 PyanNet (SincNet front end) in GEMM mode f16p, run three ways on one GPU:
  (a) one dense uvad_forward_wav_i16 per recording (B = 1 each: what the whole-recording path did before lens calls);
  (b) ragged batches packed within --max-duration padded seconds (pack_ragged_batches), one uvad_forward_wav_lens_i16 per batch;
  (c) ONE dense call padded to the longest row -- a cost reference only (its answers are wrong for every shorter row).
Checks that (b) gives every recording the bits of (a) (recurrent tile pinned to 4, mode f16p_stream for the check: f16p picks its
projection kernels by launch size).  Then times the SincNet stage alone (uvad_sincnet_lens_i16 against uvad_sincnet_i16 at the same (B, S)):
all lengths = S, and half the rows at S / 2.  One JSON line."""
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
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--stage-B", type=int, default=32)
ap.add_argument("--stage-seconds", type=float, default=60.0)
ap.add_argument("--stage-iters", type=int, default=20)
ap.add_argument("--skip-padded", action="store_true", help="leave out (c)")
args = ap.parse_args()
dev = torch.device("cuda:0")
sr = 16000
torch.manual_seed(11)
m = uvad_amd.PyanNet(); m.build(); seed_weights(m, 1234, 4.0); m = m.to(dev).eval()
rt = m.runtime(dev)
rng = np.random.default_rng(7)
nsamp = [int(v) for v in rng.uniform(args.min_seconds * sr, args.max_seconds * sr, args.recordings)]
S = max(nsamp)
pcm = torch.from_numpy(np.round(rng.standard_normal((args.recordings, S)) * 3000).clip(-32768, 32767).astype(np.int16)).to(dev)
frames = [rt.sincnet_num_frames(n) for n in nsamp]
valid = sum(frames)
batches = pack_ragged_batches(nsamp, int(args.max_duration * sr))
ragged_in = []
for grp in batches:
    n = max(nsamp[i] for i in grp)
    ragged_in.append((grp, pcm[grp, :n].contiguous(), torch.tensor([nsamp[i] for i in grp], dtype=torch.int64, device=dev)))
dense_in = [pcm[i:i + 1, :nsamp[i]].contiguous() for i in range(args.recordings)]


def run_dense():
    return [rt.forward_wav(x, want_logits=False)[1].clone() for x in dense_in]


def run_ragged():
    return [(grp, rt.forward_wav(x, want_logits=False, lengths=n)[1].clone()) for grp, x, n in ragged_in]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best, out = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


res = {"recordings": args.recordings, "min_s": args.min_seconds, "max_s": args.max_seconds, "max_duration_s": args.max_duration,
       "batches": len(batches), "valid_frames": valid}
rt.set_gemm_mode("f16p")
_, t_a = timed(run_dense, args.reps)
_, t_b = timed(run_ragged, args.reps)
res.update({"a_s": t_a, "b_s": t_b, "a_Mfps": valid / t_a / 1e6, "b_Mfps": valid / t_b / 1e6, "speedup_b_over_a": t_a / t_b})
if not args.skip_padded:
    big = pcm
    try:
        _, t_c = timed(lambda: rt.forward_wav(big, want_logits=False)[1], 1)
        res.update({"c_s": t_c, "c_Mfps_valid": valid / t_c / 1e6})
    except Exception as e:   # (a workspace of N x S samples may not fit)
        res["c_error"] = str(e)[:200]
# bit identity of (b) against (a): f16p_stream, recurrent tile pinned
rt.set_gemm_mode("f16p_stream")
rt.set_recurrent_tile(4)
a_out = run_dense()
b_out = run_ragged()
torch.cuda.synchronize()
identical, worst = True, 0.0
for grp, probs in b_out:
    for r, i in enumerate(grp):
        T = frames[i]
        g, w = probs[r, :T], a_out[i][0]
        if not torch.equal(g, w):
            identical = False
            worst = max(worst, float((g - w).abs().max()))
res.update({"b_equals_a_bits_f16p_stream": identical, "b_vs_a_max_abs": worst})
rt.set_recurrent_tile(0)
rt.set_gemm_mode("f16p")
# the SincNet stage alone, lens against dense at the same (B, S)
B2, S2 = args.stage_B, int(args.stage_seconds * sr)
x2 = pcm[:B2, :S2].contiguous() if S2 <= S and B2 <= args.recordings else torch.from_numpy(
    np.round(rng.standard_normal((B2, S2)) * 3000).astype(np.int16)).to(dev)
full = torch.full((B2,), S2, dtype=torch.int64, device=dev)
half = full.clone(); half[1::2] = S2 // 2


def stage_time(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(3):
        e0.record()
        for _ in range(args.stage_iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.stage_iters
        best = ms if best is None else min(best, ms)
    return best


t_dense = stage_time(lambda: rt.sincnet(x2))
form = rt.sincnet_form()
t_full = stage_time(lambda: rt.sincnet(x2, lengths=full))
t_half = stage_time(lambda: rt.sincnet(x2, lengths=half))
res.update({"stage_B": B2, "stage_S": S2, "stage_form": form, "stage_dense_ms": t_dense, "stage_lens_all_S_ms": t_full,
            "stage_lens_half_ms": t_half, "stage_all_S_over_dense": t_full / t_dense, "stage_half_over_dense": t_half / t_dense})
print(json.dumps(res))
