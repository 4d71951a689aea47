#!/usr/bin/env python3
"""Windowed streaming of the waveform model PyanNet (SincNet + BiLSTM head, uvad_window_wav_step): B concurrent live feeds of int16 PCM,
`chunk` samples per step, the model run from zero state over the last W frames every step (W = 293: the reference's 5 s cut in whole
frames), frames emitted L frames behind the newest complete one.
Reports p50/p99 wall latency per step (host submit -> logits visible after a synchronise), device time per step from HIP events and the
real-time factor (step wall time / audio time), timed only after the W-frame warm-up, for the step enqueued kernel by kernel and
replayed as a hipGraph.  In the same run it times the naive alternative: uvad_forward_wav_i16 on the last S_w samples every step, from a
torch-side ring.  The ring kernel's own time comes from a kernel trace of a short run (profiles/README.md)."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvad_amd
from uvad_amd.synth import seed_weights

ap = argparse.ArgumentParser()
ap.add_argument("--feeds", type=int, default=512)
ap.add_argument("--chunk", type=int, default=320)
ap.add_argument("--window", type=int, default=293)
ap.add_argument("--lookahead", type=int, default=30)
ap.add_argument("--seconds", type=float, default=60.0, help="audio per feed AFTER the warm-up")
ap.add_argument("--naive-steps", type=int, default=600)
ap.add_argument("--f32", action="store_true", help="f32 feeds instead of int16")
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(11)
m = uvad_amd.PyanNet(); m.build(); seed_weights(m, 1234, 2.0)                              # bidirectional (LSTM_DEFAULTS)
m = m.to(dev).eval()
rt = m.runtime(dev)
B, C, W, L = args.feeds, args.chunk, args.window, args.lookahead
J, R = rt.wav_window_geometry()
Sw = R + J * (W - 1)
warm = -(-(Sw + J) // C)                                                                 # steps until the window is full
steps = int(args.seconds * 16000 / C)
g = torch.Generator(device=dev); g.manual_seed(5)
audio = 0.1 * torch.randn(B, 64 * C, generator=g, device=dev)                             # 64 distinct chunks, cycled
if not args.f32:
    audio = torch.round(audio * 32767.0).clamp(-32768, 32767).to(torch.int16)
chunk_of = lambda i: audio[:, (i % 64) * C:(i % 64 + 1) * C].contiguous()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(step, n):
    lat, dev_ms, frames = [], [], 0
    for i in range(n):
        x = chunk_of(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = step(x)
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
        frames += out.shape[1]
    # a second, shorter pass with HIP events around the step (kept out of the latency loop)
    for i in range(min(n, 300)):
        x = chunk_of(i)
        torch.cuda.synchronize()
        e0.record()
        step(x)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    lat = np.array(lat) * 1e3
    audio_s = n * C / 16000.0
    return {"steps": n, "frames_per_feed": frames, "p50_ms": float(np.percentile(lat, 50)), "p99_ms": float(np.percentile(lat, 99)),
            "max_ms": float(lat.max()), "device_ms_p50": float(np.percentile(dev_ms, 50)), "rtf": float(lat.sum() / 1e3 / audio_s)}


res = {"config": f"{B} {'f32' if args.f32 else 'int16'} feeds x {C}-sample chunks, W = {W} frames ({Sw} samples), L = {L}, "
                 f"PyanNet (SincNet J = {J}, R = {R}, bidirectional head), {steps * C / 16000.0:.0f} s of audio per feed timed after a "
                 f"{warm}-step warm-up"}
for graphs in (False, True):
    st = rt.wav_window_stream_open(B, C, window=W, lookahead=L, graphs=graphs, dtype=audio.dtype)
    for i in range(warm):
        rt.wav_window_stream_step(st, chunk_of(i))
    torch.cuda.synchronize()
    r = timed(lambda x: rt.wav_window_stream_step(st, x), steps)
    if graphs:
        r["graphs"] = len(st["graphs"])
    r["time_chunks"] = rt.time_chunks()
    r["sincnet_form"] = rt.sincnet_form()
    res["window_graphs" if graphs else "window"] = r
    del st

# naive: the last S_w samples in a torch-side ring, uvad_forward_wav(_i16) on all of them every step
ring = torch.zeros(B, 2 * Sw, dtype=audio.dtype, device=dev)
pos = [0]


def naive(x):
    p = pos[0] % Sw
    n1 = min(C, Sw - p)
    ring[:, p:p + n1] = x[:, :n1]
    ring[:, p + Sw:p + Sw + n1] = x[:, :n1]                               # mirrored copy: the last S_w samples are one contiguous slice
    if n1 < C:
        ring[:, :C - n1] = x[:, n1:]
        ring[:, Sw:Sw + C - n1] = x[:, n1:]
    pos[0] += C
    q = pos[0] % Sw
    lg, _ = rt.forward_wav(ring[:, q:q + Sw], want_probs=False)
    k = -(-C // J)                                                        # at most ceil(C / J) frames complete per step
    return lg[:, -k:]


rt.set_time_chunks(1)                                                    # as the stream runs the classifier
for i in range(warm):
    naive(chunk_of(i))
torch.cuda.synchronize()
res["naive_forward_wav_last_window"] = timed(naive, min(steps, args.naive_steps))
res["stream_vs_naive_p50"] = res["window"]["p50_ms"] / res["naive_forward_wav_last_window"]["p50_ms"]
res["what"] = ("p50_ms = host wall time of one step (submit -> synchronised); device_ms = HIP events around the step; rtf = summed step wall "
               "time / audio time; naive = uvad_forward_wav on the last S_w samples every step from a torch-side ring, time chunks 1")
print(json.dumps(res))
