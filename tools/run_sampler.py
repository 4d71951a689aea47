"""Measure the sampler stage (uvad_sampler_step) on one GPU in one run, candidates alternated block by block: the graph replay time of one
step of 256 rows x 80 000 samples from an f32 and an int16 corpus (waveform label grid, pad) and at the log-mel training shape (log-mel label
grid, per-row lengths); the gather's effective bandwidth (bytes read + bytes written over the step time) beside the float4 copy rate
recorded in profiles/cuts.json; the waveform train step (SincNet + 4 LSTM layers + head, forward, backward, Adam: one graph replay) alone
and with the sampler in front of it; and, on the wall clock, the host batch assembly the sampler replaces (train_vad's torch.stack of row
slices and torch.cat of label rows over the same windows).  Writes profiles/sampler.json.
Usage: python tools/run_sampler.py [--blocks 7] [--reps 20] [--train-reps 2] [--no-train] [--out profiles/sampler.json]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def copy_rate_tbs():
    """The float4 copy rate profiles/cuts.json was measured against (it is part of that file's key names)."""
    text = open(os.path.join(ROOT, "profiles", "cuts.json")).read()
    return float(re.search(r"hbm_copy_rate_([0-9.]+)TBs", text).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train-reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler.json"))
    a = ap.parse_args()
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    B, W, R, sr = a.batch, 80000, 64, 16000
    m = uvad_amd.PyanNet()                                                # 4 x 128 bidirectional, head 128 / 2, the reference's SincNet
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    m2 = uvad_amd.PyanNet2(encoding_dim=80)
    m2.build()
    m2.attach_fbank(uvad_amd.FbankConfig(num_filters=80))
    rt2 = m2.to(dev).eval().runtime(dev)

    g = torch.Generator().manual_seed(1)
    lens = [int(v) for v in torch.randint(20 * sr, 120 * sr, (R,), generator=g)]          # odd lengths: three of four source offsets are not 16-byte aligned
    corpus = 0.1 * torch.randn(sum(lens), generator=g)
    corpus16 = (corpus * 32767.0).round().to(torch.int16)
    rng = np.random.default_rng(2)
    sups = []
    for n in lens:                                                         # about one supervision per three seconds
        k = max(1, n // (3 * sr))
        s = np.sort(rng.integers(0, n, k))
        sups.append(np.stack([s, s + rng.integers(sr // 4, 2 * sr, k)], 1))
    sets, weights = [r % 3 for r in range(R)], (1.0, 2.0, 5.0)

    cands, moved, states = {}, {}, {}
    for name, r, pcm, geometry, pad, keep in (("sampler_f32_wav_grid", rt, corpus, "sincnet", True, 3 * sr), ("sampler_i16_wav_grid", rt, corpus16, "sincnet", True, 3 * sr),
                                              ("sampler_f32_logmel_grid", rt2, corpus, "fbank", False, 3 * sr)):
        st = r.sampler_open(pcm, lens, sups, W, keep, geometry, datasets=sets, weights=weights, pad=pad, seed=0x5EED)
        res = r.sampler_step(st, B, cursor=[0, 0, 0], draw=0)             # the buffers of this batch size; no state update
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            r.sampler_step(st, B)
        cands[name], states[name] = gr.replay, (r, st, res)
        moved[name] = B * W * (4 + pcm.element_size())                    # full windows; the labels and the plan are below a percent of it

    # the host assembly of the same windows: the rows train_vad stacked per batch, with label rows rasterised once at set-up
    r, st, res = states["sampler_f32_wav_grid"]
    plan = r.sampler_step(st, B, plan=True, cursor=[0, 0, 0], draw=0)["plan"].cpu().numpy()
    first = np.concatenate([[0], np.cumsum(lens)])
    dev_corpus = corpus.to(dev)
    T = int(res["labels"].shape[1])
    label_rows = [torch.zeros((1, T), dtype=torch.uint8, device=dev) for _ in range(B)]
    picks = [(int(first[p[4]] + p[5]), int(p[6])) for p in plan]

    def host_batch():
        x = torch.zeros((B, W), dtype=torch.float32, device=dev)
        for i, (s0, n) in enumerate(picks):
            x[i, :n] = dev_corpus[s0:s0 + n]
        return x, torch.cat(label_rows)
    host_ms = []
    for _ in range(a.blocks + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_batch()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    host_ms = host_ms[2:]

    train = {"measured": False}
    if not a.no_train:
        try:
            hh, hl, hs = rt.head_train_open(), rt.lstm_train_open(layers=m.hparams.lstm["num_layers"]), rt.sincnet_train_open()
            fixed = res["pcm"].clone()
            y = res["labels"].clone()

            def step(sample):
                src, gt = fixed, y
                if sample:
                    got = rt.sampler_step(st, B)
                    src, gt = got["pcm"], got["labels"]
                f = rt.sincnet_train_forward(hs, src)
                o = rt.lstm_train_forward(hl, f)
                _, gx = rt.head_train_grad(hh, o, gt, want_grad_x=True)
                gin = rt.lstm_train_backward(hl, f, gx, want_grad_in=True)
                rt.sincnet_train_backward(hs, src, gin)
                rt.head_train_apply(hh), rt.lstm_train_apply(hl), rt.sincnet_train_apply(hs)
            for sample, name in ((False, "train_step"), (True, "sampler_and_train_step")):
                step(sample)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    step(sample)
                cands[name] = gr.replay
            train["measured"] = True
        except Exception as e:                                            # the stage's numbers stand without it; the file says why
            train["error"] = f"{type(e).__name__}: {e}"[:300]

    reps = {k: a.train_reps if "train_step" in k else a.reps for k in cands}
    for fn in cands.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(a.blocks):                                             # alternated blocks: drift and clock state hit every candidate alike
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[k]):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps[k])
    rate = copy_rate_tbs()
    out = {"shape": {"B": B, "W": W, "recordings": R, "corpus_samples": sum(lens), "supervisions": int(sum(len(s) for s in sups)), "datasets": 3},
           "method": f"HIP events around blocks of {a.reps} graph replays ({a.train_reps} for the train steps), {a.blocks} blocks per candidate, candidates "
                     "alternated block by block in one process; the host assembly on the wall clock with a synchronisation on both sides",
           "device": torch.cuda.get_device_name(0), "float4_copy_rate_tbs_from_profiles_cuts_json": rate, "train": train,
           "host_batch_assembly": {"ms_median": float(np.median(host_ms)), "ms_min": float(min(host_ms)), "ms_max": float(max(host_ms)),
                                   "what": "torch.zeros + 256 row-slice copies + torch.cat of 256 label rows, labels rasterised beforehand"}}
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()), "blocks_ms": [round(float(t), 4) for t in v]}
        if k in moved:
            tbs = moved[k] / (out[k]["ms_median"] * 1e-3) / 1e12
            out[k].update({"bytes_moved": moved[k], "tbs_over_step_time": tbs, "share_of_float4_copy_rate": tbs / rate})
    if train["measured"]:
        t0, t1 = out["train_step"], out["sampler_and_train_step"]
        out["sampler_cost_in_train_step_ms"] = t1["ms_median"] - t0["ms_median"]
        out["sampler_share_of_train_step"] = out["sampler_cost_in_train_step_ms"] / t0["ms_median"]
        out["ranges_resolve"] = bool(t1["ms_min"] > t0["ms_max"] or t1["ms_max"] < t0["ms_min"])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (round(v["ms_median"], 4), round(v.get("tbs_over_step_time", 0.0), 3)) for k, v in out.items()
                      if isinstance(v, dict) and "ms_median" in v}))
    print(json.dumps({k: out.get(k) for k in ("sampler_cost_in_train_step_ms", "sampler_share_of_train_step", "ranges_resolve", "train")}))


if __name__ == "__main__":
    main()
