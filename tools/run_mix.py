"""Measure the noise-mixing stage (uvad_mix_step) at 256 x 80 000 samples on one GPU in one run: the graph replay time of one step from
f32 (out of place and in place) and from int16, with mix_prob 0.5 and 1.0, over batches taken in rotation (four graphs on four buffer
sets, 650 MB together, so that no replay finds its batch in a cache), the effective bandwidth beside the float4 copy of
profiles/cuts.json, and the step's share of a waveform train_step (SincNet + 4 LSTM layers + head, forward, backward, Adam: one graph
replay) at the same batch: the train step alone and the mix in front of it, alternated block by block, median and spread over the
blocks.  The noise bank is 64 clips of 1 to 30 s.  Writes profiles/mix.json.
Usage: python tools/run_mix.py [--blocks 9] [--reps 10] [--train-reps 2] [--out profiles/mix.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBS = 6.29        # float4 copy on this GPU: profiles/cuts.json


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--train-reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix.json"))
    a = ap.parse_args()
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    B, S, NB = a.batch, 80000, 4
    m = uvad_amd.PyanNet()                                                # 4 x 128 bidirectional, head 128 / 2, the reference's SincNet
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(dev).eval()
    rt = m.runtime(dev)
    g = torch.Generator().manual_seed(1)
    clip_lengths = [int(v) for v in torch.randint(16000, 480000, (64,), generator=g)]
    bank = 0.05 * torch.randn(sum(clip_lengths), generator=g)
    wav = [(0.1 * torch.randn(B, S, generator=g)).to(dev) for _ in range(NB)]
    wav16 = [(w * 32767.0).round().to(torch.int16) for w in wav]
    outs = [torch.empty(B, S, device=dev) for _ in range(NB)]

    cands, states = {}, {}
    turn = [0]

    def rotating(graphs):
        def fn():
            turn[0] += 1
            graphs[turn[0] % NB].replay()
        return fn
    for name, p, src, inplace in (("mix_f32_p05", 0.5, wav, False), ("mix_f32_p1", 1.0, wav, False), ("mix_f32_in_place_p05", 0.5, wav, True),
                                  ("mix_i16_p05", 0.5, wav16, False), ("mix_i16_p1", 1.0, wav16, False)):
        st = rt.mix_open(bank, clip_lengths, snr=(10, 20), mix_prob=p, seed=0x5EED)
        bufs = [w.clone() for w in src] if inplace else src
        rt.mix_step(st, bufs[0], out=bufs[0] if inplace else outs[0])     # sizes the workspace
        torch.cuda.synchronize()
        graphs = []
        for k in range(NB):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                rt.mix_step(st, bufs[k], out=bufs[k] if inplace else outs[k])
            graphs.append(gr)
        cands[name], states[name] = rotating(graphs), st

    train = {"measured": False}
    try:
        T = m.num_frames(S)
        y = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8).to(dev)
        L = m.hparams.lstm["num_layers"]
        hh, hl, hs = rt.head_train_open(), rt.lstm_train_open(layers=L), rt.sincnet_train_open()
        st = rt.mix_open(bank, clip_lengths, snr=(10, 20), mix_prob=0.5, seed=0x5EED)
        x = wav[0].clone()

        def step(mix):
            src = rt.mix_step(st, wav[0], out=x) if mix else wav[0]
            f = rt.sincnet_train_forward(hs, src)
            o = rt.lstm_train_forward(hl, f)
            _, gx = rt.head_train_grad(hh, o, y, want_grad_x=True)
            gin = rt.lstm_train_backward(hl, f, gx, want_grad_in=True)
            rt.sincnet_train_backward(hs, src, gin)
            rt.head_train_apply(hh), rt.lstm_train_apply(hl), rt.sincnet_train_apply(hs)
        for mix, name in ((False, "train_step"), (True, "mix_and_train_step")):
            step(mix)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                step(mix)
            cands[name] = gr.replay
        states["mix_and_train_step"] = st
        train["measured"] = True
    except Exception as e:                                                # the mix numbers stand without it; the file says why
        train["error"] = f"{type(e).__name__}: {e}"[:300]

    reps = {k: a.train_reps if "train_step" in k else a.reps for k in cands}
    for fn in cands.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    draws0 = {k: rt.mix_draws(s) for k, s in states.items()}
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
    out = {"shape": {"B": B, "S": S, "clips": len(clip_lengths), "bank_samples": sum(clip_lengths), "snr_steps": 1024, "max_seg": 8},
           "method": f"HIP events around blocks of {a.reps} graph replays ({a.train_reps} for the train steps), {a.blocks} blocks per candidate, candidates "
                     f"alternated block by block in one process; each mix candidate rotates over {NB} graphs on {NB} batches",
           "device": torch.cuda.get_device_name(0), "draws_while_timed": {k: rt.mix_draws(s) - draws0[k] for k, s in states.items()},
           "float4_copy_tb_per_s": COPY_TBS, "train": train}
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()), "blocks_ms": [round(float(t), 4) for t in v]}
    # bytes the launches move per sample: the energy pass reads the row (4 / 2); the mix pass reads it again and writes f32 (4 / 2 + 4), and
    # reads 4 bytes of noise per mixed sample; in place, rows that are not mixed are not touched by the mix pass
    for name, in_b, p, inplace in (("mix_f32_p05", 4, 0.5, False), ("mix_f32_p1", 4, 1.0, False), ("mix_f32_in_place_p05", 4, 0.5, True),
                                   ("mix_i16_p05", 2, 0.5, False), ("mix_i16_p1", 2, 1.0, False)):
        per = in_b + (p if inplace else 1.0) * (in_b + 4) + p * 4
        nbytes = per * B * S
        out[name].update({"bytes_per_sample": per, "bytes_per_call": int(nbytes), "tb_per_s": nbytes / (out[name]["ms_median"] * 1e-3) / 1e12})
        out[name]["fraction_of_float4_copy"] = out[name]["tb_per_s"] / COPY_TBS
    if train["measured"]:
        t0, t1 = out["train_step"], out["mix_and_train_step"]
        out["mix_cost_in_train_step_ms"] = t1["ms_median"] - t0["ms_median"]
        out["mix_share_of_train_step"] = out["mix_cost_in_train_step_ms"] / t0["ms_median"]
        out["ranges_resolve"] = bool(t1["ms_min"] > t0["ms_max"] or t1["ms_max"] < t0["ms_min"])
        out["mix_alone_share_of_train_step"] = out["mix_f32_p05"]["ms_median"] / t0["ms_median"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (round(v["ms_median"], 4), round(v.get("tb_per_s", 0.0), 3)) for k, v in out.items() if isinstance(v, dict) and "ms_median" in v}))
    print(json.dumps({k: out.get(k) for k in ("mix_cost_in_train_step_ms", "mix_share_of_train_step", "ranges_resolve", "train")}))


if __name__ == "__main__":
    main()
