#!/usr/bin/env python3
"""PyanNet (SincNet front end) frames/s with several batches in flight (ForwardPipeline over uvad_forward_wav[_i16]) and with int16
waveform ingest.  Prints ONE JSON line.

Measured, per shape (256 x 5 s and the reference's 80 x 5 s, 293 frames per cut), for f32 and int16 input batches resident on the
device:
  * one batch at a time: VadRuntime.forward_wav, recurrent_tile 0 (the library's per-call choice) and 16;
  * depth d in {2, 4, 8, 12} in flight: one ForwardPipeline of depth 12, its slots set to recurrent_tile 16 or 0, set_active_depth(d).
Timing: every configuration is warmed up, then `--steps` steps are bracketed by device events on the caller's stream (the pipeline's
streams wait for the start event and the end event waits for all of them); the median of `--reps` windows is reported.
Host side (what predict_vad does per batch): an int16 batch in host memory -> device -> PyanNet probabilities, (a) converted with torch
on the device (x.float() / 32768, the previous flow) and (b) sent to uvad_forward_wav_i16 as it is; host clock around work that ends
in a synchronise, alternating (a) and (b).
--trace: a warm-up call, then one uvad_forward_wav call and one uvad_forward_wav_i16 call (inputs copied from the host, so no torch
kernel runs except the fills that separate the calls), for `rocprofv3 --kernel-trace --stats -- python tools/run_sincnet_inflight.py --trace`;
--summarize-trace CSV lists the kernels of each call from that trace's kernel_trace.csv.
Before the first HIP call GPU_MAX_HW_QUEUES defaults to 16 (as bench.py): twelve steps in flight need one hardware queue each."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEPTHS = (2, 4, 8, 12)


def summarize_trace(path):
    """kernel_trace.csv of a --trace run: the dispatches between the torch fill kernels that separate the calls (the first segment is the
    warm-up call), each call's dispatches up to the first torch kernel after it; the resources rocprofv3 reports per dispatch."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    segs, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "FillFunctor" in name:
            if cur is not None:
                segs.append(cur)
            cur = []
        elif cur is not None:
            cur.append(r)
    if cur is not None:
        segs.append(cur)
    calls = []
    for seg in segs:
        ks = []
        for r in seg:
            if "at::native" in r["Kernel_Name"]:
                break
            ks.append(r)
        calls.append(ks)
    short = lambda n: n.replace("void ", "").replace("uvad::(anonymous namespace)::", "").split("(")[0]
    out = {"calls": [{"dispatches": len(c), "kernel_us_total": round(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in c) / 1e3, 1),
                      "kernels": [short(r["Kernel_Name"]) for r in c]} for c in calls]}
    if len(calls) == 2:
        strip = lambda k: k.replace("wav_stats_i16_kernel", "wav_stats_kernel").replace("<1, true>", "<1, false>")
        out["same_kernel_sequence_modulo_sample_type"] = [strip(k) for k in out["calls"][0]["kernels"]] == [strip(k) for k in out["calls"][1]["kernels"]]
        out["waveform_kernels"] = {short(r["Kernel_Name"]): {"us": round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 1),
                                                             "vgpr": int(r["VGPR_Count"]), "agpr": int(r["Accum_VGPR_Count"]),
                                                             "scratch": int(r["Scratch_Size"])}
                                   for c in calls for r in c[:2]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48, help="steps per timed window")
    ap.add_argument("--reps", type=int, default=3, help="timed windows per configuration (median reported)")
    ap.add_argument("--warmup", type=int, default=8, help="untimed steps before each configuration")
    ap.add_argument("--shapes", default="256x80000,80x80000", help="comma-separated BxS")
    ap.add_argument("--host-reps", type=int, default=20, help="host-path iterations per variant")
    ap.add_argument("--trace", action="store_true", help="one uvad_forward_wav and one uvad_forward_wav_i16 call only (for rocprofv3)")
    ap.add_argument("--summarize-trace", default=None, help="kernel_trace.csv of a --trace run -> JSON summary")
    args = ap.parse_args()
    if args.summarize_trace:
        summarize_trace(args.summarize_trace)
        return

    import numpy as np
    import torch
    import uvad_amd
    from uvad_amd.synth import seed_weights, synth_pcm, synth_pcm_device

    dev = torch.device("cuda:0")
    torch.manual_seed(1234)   # the SincNet convolutions keep torch's default initialisation: seeded (as tools/run_sincnet.py)
    m = uvad_amd.PyanNet()
    m.build()
    seed_weights(m, 1234, 4.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)

    if args.trace:
        q = np.round(synth_pcm(256, 80000, seed=5) * 32767.0).astype(np.int16)
        xf = torch.from_numpy(q.astype(np.float32) / 32768.0).to(dev)
        xq = torch.from_numpy(q).to(dev)
        rt.forward_wav(xf, want_probs=False)   # warm-up: first-call work (kernel attributes, the side-stream probe of time chunking)
        calls = []
        for x in (xf, xq):
            torch.cuda.synchronize()
            torch.zeros(1, device=dev)         # separator in the trace
            torch.cuda.synchronize()
            calls.append(rt.forward_wav(x, want_probs=False)[0])
            torch.cuda.synchronize()
        print(json.dumps({"trace": "warm-up, then forward_wav (f32) and forward_wav_i16 on the same samples, B=256 x 80000",
                          "bit_identical": bool(torch.equal(calls[0], calls[1]))}))
        return

    def window(fn_steps):
        """device time (ms) of fn_steps() bracketed by events on the current stream"""
        cur = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(cur)
        fn_steps()
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1)

    result = {"tool": "run_sincnet_inflight", "model": "PyanNet (default-init SincNet + seeded x4 classifier), GEMM mode f16p",
              "steps": args.steps, "reps": args.reps, "warmup": args.warmup,
              "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "frames_per_s": {}, "bit_identical": {}}
    pipe = None
    try:
        depths = list(DEPTHS)
        while pipe is None:   # the deepest pipeline the device's hardware queues allow (GPU_MAX_HW_QUEUES set lower by the caller)
            try:
                pipe = uvad_amd.ForwardPipeline(m, dev, depth=depths[-1], recurrent_tile=16)
            except RuntimeError as e:
                if "concurrent HIP streams" not in str(e) or len(depths) == 1:
                    raise
                depths.pop()
        result["streams_tried"] = pipe.streams_tried
        result["depths"] = depths
        for shape in args.shapes.split(","):
            B, S = (int(v) for v in shape.split("x"))
            T = rt.sincnet_num_frames(S)
            nb = max(DEPTHS)   # distinct input batches, one per slot at the deepest setting
            inputs = {"i16": [torch.round(synth_pcm_device(B, S, 100 * i + 1, dev) * 32767.0).to(torch.int16) for i in range(nb)]}
            inputs["f32"] = [x.float() / 32768.0 for x in inputs["i16"]]
            torch.cuda.synchronize()
            res = {}
            for kind, xs in inputs.items():
                r = {}
                for tile in (0, 16):   # one batch at a time
                    rt.set_recurrent_tile(tile)
                    run = lambda n: [rt.forward_wav(xs[k % nb], want_probs=False) for k in range(n)]
                    run(args.warmup)
                    ms = statistics.median(window(lambda: run(args.steps)) for _ in range(args.reps))
                    r[f"seq_tile{tile}"] = round(B * T * args.steps / ms * 1e3 / 1e6, 2)
                rt.set_recurrent_tile(0)
                for tile in (16, 0):
                    for r_ in pipe.runtimes:
                        r_.set_recurrent_tile(tile)
                    for d in depths:
                        pipe.set_active_depth(d)
                        cur = torch.cuda.current_stream(dev)

                        def run(n):
                            for k in range(n):
                                pipe.submit(xs[k % nb], want_logits=True, want_probs=False)
                            for s in pipe.streams[:d]:
                                cur.wait_stream(s)
                        run(args.warmup)
                        ms = statistics.median(window(lambda: run(args.steps)) for _ in range(args.reps))
                        r[f"d{d}_tile{tile}"] = round(B * T * args.steps / ms * 1e3 / 1e6, 2)
                res[kind] = r
            # the pipelined int16 results are the sequential f32 bits on q / 32768 (same recurrent form)
            for r_ in pipe.runtimes:
                r_.set_recurrent_tile(16)
            pipe.set_active_depth(4)
            rt.set_recurrent_tile(16)
            want = [rt.forward_wav(inputs["f32"][k])[0].clone() for k in range(4)]
            rt.set_recurrent_tile(0)
            got = [p.result()[0] for p in [pipe.submit(inputs["i16"][k]) for k in range(4)]]
            result["bit_identical"][shape] = all(torch.equal(a, b) for a, b in zip(want, got))
            result["frames_per_s"][f"{B}x{S / 16000:g}s"] = {"unit": "M frames/s", "frames_per_batch": B * T, **res}
            del inputs
            torch.cuda.synchronize()
        # host side, as predict_vad: int16 batch in (pageable) host memory -> device -> probabilities
        B, S = 256, 80000
        qh = torch.round(synth_pcm_device(B, S, 7, dev) * 32767.0).to(torch.int16).cpu()   # pageable host memory, as a wav file's samples
        variants = {"torch_convert_then_f32": lambda: rt.forward_wav(qh.to(dev).float() / 32768.0, want_logits=False),
                    "int16_unconverted": lambda: rt.forward_wav(qh.to(dev), want_logits=False)}
        times = {k: [] for k in variants}
        for k, fn in variants.items():
            fn(); fn()
        torch.cuda.synchronize()
        for _ in range(args.host_reps):
            for k, fn in variants.items():   # alternating
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        result["host_path_256x5s_ms"] = {k: round(statistics.median(v), 3) for k, v in times.items()}
        result["host_path_256x5s_ms_min"] = {k: round(min(v), 3) for k, v in times.items()}
    finally:
        if pipe is not None:
            pipe.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
