"""Measure the reverberation stage (uvad_reverb_step) at 256 x 80 000 samples on one GPU in one run: the graph replay time of one step
from f32 and int16 rows with a bank of 64 synthetic responses (synth.rir) of K = 4 000 and 8 000 taps, prob 0.5 and 1, alternated
block by block with uvad_mix_step and with the waveform train step the stage precedes (SincNet + 4 LSTM layers + head, forward,
backward, Adam: one graph replay), alone and with reverb -> mix in front of it.  The algorithmic work is 2 sum_{drawn rows} n_b K_r
FLOP: exact at prob 1 (every row is drawn), the expectation at prob 0.5.  For information, the row-normwise error max|z - z64| / rms(z64)
of one row at K = 8 000 beside torch.nn.functional.conv1d in f32 on the CPU.  Writes profiles/reverb.json.
Usage: python tools/run_reverb.py [--blocks 7] [--reps 10] [--train-reps 2] [--no-train] [--out profiles/reverb.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_MATRIX_PEAK_TF = 157.3     # v_mfma_f32_32x32x2_f32, the spec figure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--train-reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverb.json"))
    a = ap.parse_args()
    import uvad_amd
    from uvad_amd.synth import rir, seed_weights
    dev = torch.device("cuda:0")
    B, S, R = a.batch, 80000, 64
    m = uvad_amd.PyanNet()                                                # 4 x 128 bidirectional, head 128 / 2, the reference's SincNet
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    g = torch.Generator().manual_seed(1)
    wav = (0.1 * torch.randn(B, S, generator=g)).to(dev)
    wav16 = (wav * 32767.0).round().to(torch.int16)
    out_buf = torch.empty(B, S, device=dev)
    banks = {K: np.concatenate([rir(K, 0.5, 10 + r, seed=r) for r in range(R)]) for K in (4000, 8000)}

    cands, states, work = {}, {}, {}
    for name, K, p, src in (("reverb_f32_k4000_p05", 4000, 0.5, wav), ("reverb_f32_k4000_p1", 4000, 1.0, wav), ("reverb_f32_k8000_p05", 8000, 0.5, wav),
                            ("reverb_f32_k8000_p1", 8000, 1.0, wav), ("reverb_i16_k8000_p1", 8000, 1.0, wav16)):
        st = rt.reverb_open(banks[K], [K] * R, prob=p, normalize=True, align=True, seed=0x5EED)
        rt.reverb_step(st, src, out=out_buf)                              # sizes the workspace
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            rt.reverb_step(st, src, out=out_buf)
        cands[name], states[name], work[name] = gr.replay, st, 2.0 * p * B * S * K

    # for information: the error of one row at K = 8 000 against float64, beside torch's f32 conv1d on the CPU
    st = rt.reverb_open(banks[8000][:8000], [8000], prob=1.0, normalize=False, align=False, seed=1)
    z = rt.reverb_step(st, wav[:1], draw=0)[0].cpu().numpy().astype(np.float64)
    x64, h64 = wav[0].cpu().numpy().astype(np.float64), banks[8000][:8000].astype(np.float64)
    z64 = np.convolve(x64, h64)[:S]
    zt = torch.nn.functional.conv1d(wav[:1, None].cpu(), torch.from_numpy(banks[8000][:8000].copy()).flip(0)[None, None], padding=7999)[0, 0, :S]
    rms = float(np.sqrt(np.mean(z64 * z64)))
    error = {"K": 8000, "S": S, "device_max_err_over_rms": float(np.abs(z - z64).max() / rms),
             "torch_conv1d_f32_cpu_max_err_over_rms": float(np.abs(zt.numpy().astype(np.float64) - z64).max() / rms)}

    gm = torch.Generator().manual_seed(2)
    clip_lengths = [int(v) for v in torch.randint(16000, 480000, (64,), generator=gm)]
    mix = rt.mix_open(0.05 * torch.randn(sum(clip_lengths), generator=gm), clip_lengths, snr=(10, 20), mix_prob=0.5, seed=0x5EED)
    rt.mix_step(mix, wav, out=out_buf)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        rt.mix_step(mix, wav, out=out_buf)
    cands["mix_f32_p05"] = gr.replay

    train = {"measured": False}
    if not a.no_train:
        try:
            T = m.num_frames(S)
            y = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8).to(dev)
            hh, hl, hs = rt.head_train_open(), rt.lstm_train_open(layers=m.hparams.lstm["num_layers"]), rt.sincnet_train_open()
            rv = rt.reverb_open(banks[8000], [8000] * R, prob=0.5, normalize=True, align=True, seed=0x5EED)
            mx = rt.mix_open(0.05 * torch.randn(sum(clip_lengths), generator=gm), clip_lengths, snr=(10, 20), mix_prob=0.5, seed=0x5EED)
            x = torch.empty(B, S, device=dev)

            def step(augment):
                src = wav
                if augment:
                    src = rt.reverb_step(rv, wav, out=x)
                    rt.mix_step(mx, x, out=x)
                f = rt.sincnet_train_forward(hs, src)
                o = rt.lstm_train_forward(hl, f)
                _, gx = rt.head_train_grad(hh, o, y, want_grad_x=True)
                gin = rt.lstm_train_backward(hl, f, gx, want_grad_in=True)
                rt.sincnet_train_backward(hs, src, gin)
                rt.head_train_apply(hh), rt.lstm_train_apply(hl), rt.sincnet_train_apply(hs)
            for augment, name in ((False, "train_step"), (True, "reverb_mix_and_train_step")):
                step(augment)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    step(augment)
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
    out = {"shape": {"B": B, "S": S, "rirs": R, "normalize": True, "align": True},
           "method": f"HIP events around blocks of {a.reps} graph replays ({a.train_reps} for the train steps), {a.blocks} blocks per candidate, candidates "
                     "alternated block by block in one process",
           "device": torch.cuda.get_device_name(0), "f32_matrix_peak_tflops": F32_MATRIX_PEAK_TF, "error_for_information": error, "train": train}
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()), "blocks_ms": [round(float(t), 4) for t in v]}
        if k in work:
            tf = work[k] / (out[k]["ms_median"] * 1e-3) / 1e12
            out[k].update({"algorithmic_flop": work[k], "tflops_over_step_time": tf, "fraction_of_f32_matrix_peak": tf / F32_MATRIX_PEAK_TF})
    if train["measured"]:
        t0, t1 = out["train_step"], out["reverb_mix_and_train_step"]
        out["augment_cost_in_train_step_ms"] = t1["ms_median"] - t0["ms_median"]
        out["augment_share_of_train_step"] = out["augment_cost_in_train_step_ms"] / t0["ms_median"]
        out["ranges_resolve"] = bool(t1["ms_min"] > t0["ms_max"] or t1["ms_max"] < t0["ms_min"])
        out["reverb_alone_share_of_train_step"] = out["reverb_f32_k8000_p05"]["ms_median"] / t0["ms_median"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (round(v["ms_median"], 4), round(v.get("tflops_over_step_time", 0.0), 2)) for k, v in out.items()
                      if isinstance(v, dict) and "ms_median" in v}))
    print(json.dumps({k: out.get(k) for k in ("augment_cost_in_train_step_ms", "augment_share_of_train_step", "ranges_resolve", "error_for_information",
                                              "train")}))


if __name__ == "__main__":
    main()
