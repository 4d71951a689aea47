"""GPU tests (-m gpu) of the speech gate behind both slot pools (window_slots_open / wav_window_slots_open with endpoint=..., gate=...): the
gate's step is enqueued behind the endpointer's -- inside the one captured graph under graphs=True -- on the pool's input chunk, the
endpointer's labels and the pool's flags.  B = 4 slots, window 32; the log-mel pool steps its smallest legal chunk (120 samples, f32), the
waveform pool one frame step (270 samples, int16: a smaller chunk is legal there, but at one sample per step a session of a few frames
would take thousands of steps).  Three overlapping sessions, one of them restarted without END, and a one-step session.  The gated audio
of every ended session equals speech_cuts on that session's own finalised labels and PCM; every step equals tests/gate_ref.py on the
labels the run itself emitted; no record is LOST or SHORT with the default geometry; and the pool's probabilities, events and labels are
bit-identical to the same pool opened without the gate."""
import numpy as np
import pytest
import torch

import gate_ref as gr
import test_gpu_endpoint_slots as es

pytestmark = pytest.mark.gpu

DEV = es.DEV
STEPS, B, W, L = 64, 4, 32, 3
_INTS = {"min_on": 3, "min_off": 2, "pad_on": 1, "pad_off": 2}
KEYS = ("pad", "max_len", "min_len", "hop", "lead", "tail")
EP_OUT = ("events", "ev_counts", "active", "labels", "lab_counts")


def _flags():
    """Slot 0 from step 0 to 40; slot 1 from 5, restarted at 25 while busy, ended at 50; slot 3 a one-step session at 6 and one from 9 to
    58; slot 2 stays idle."""
    f = np.zeros((STEPS, B), np.uint8)
    f[0, 0], f[40, 0] = 1, 2
    f[5, 1], f[25, 1], f[50, 1] = 1, 1, 2
    f[6, 3], f[9, 3], f[58, 3] = 3, 1, 2
    return f


def _pcm(chunk, seed, dtype):
    """Bursts of noise and silence, a few chunks each, different per slot; NaN (f32) in the idle slot's rows."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, STEPS * chunk), np.float32)
    for b in range(B):
        pos, loud = 0, bool(b % 2)
        while pos < x.shape[1]:
            n = int(rng.integers(4, 16)) * chunk
            if loud:
                x[b, pos:pos + n] = 0.3 * rng.standard_normal(min(n, x.shape[1] - pos)).astype(np.float32)
            pos, loud = pos + n, not loud
    if dtype == torch.int16:
        return torch.from_numpy(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)).to(DEV)
    x[2] = np.nan
    return torch.from_numpy(x).to(DEV)


def _run(open_pool, step, x, flags, chunk, endpoint, gate, graphs):
    st = open_pool(endpoint=endpoint, gate=gate, graphs=graphs)
    out = []
    for s in range(STEPS):
        fl = flags[s]
        xs = x[:, s * chunk:(s + 1) * chunk].contiguous()
        lg, cnt = step(st, xs, start=fl & 1 == 1, end=fl & 2 == 2) if fl.any() else step(st, xs)
        rec = {"logits": lg.clone(), "counts": cnt.clone()}
        if endpoint is not None:
            rec.update(probs=st["probs"].clone(), **{k: st["endpoint"][k].clone() for k in EP_OUT})
        if gate is not None:
            rec.update({k: st["gate"][k].clone() for k in ("out", "seg", "seg_counts")})
        out.append(rec)
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in rec.items()} for rec in out], st


def _sessions(flags):
    """(slot, first step, last step) of the sessions that START and END."""
    out = []
    for b in range(flags.shape[1]):
        s0 = None
        for s in range(flags.shape[0]):
            if flags[s, b] & 1:
                s0 = s
            if flags[s, b] & 2 and s0 is not None:
                out.append((b, s0, s))
                s0 = None
    return out


def _check(rt, open_pool, step, x, chunk, endpoint, gate, geometry, ep_lag):
    flags = _flags()
    hop, lead, tail = geometry
    cfg = (gate.get("pad", 0), gate.get("max_len", 0), 0, hop, lead, tail)
    lag = L + ep_lag + -(-tail // hop)
    xs = x.cpu().numpy()
    for graphs in (False, True):
        plain, st0 = _run(open_pool, step, x, flags, chunk, endpoint, None, graphs)
        got, st = _run(open_pool, step, x, flags, chunk, endpoint, gate, graphs)
        assert "gate" not in st0
        if graphs:
            assert st["graphs"] == 1                                        # pool step, endpoint step and gate step in the one capture
        g = st["gate"]
        assert tuple(getattr(g["cfg"], k) for k in KEYS) == cfg and g["lag_frames"] == lag and g["history"] == gr.history(cfg, lag, chunk)
        assert g["ld_lab"] == st["endpoint"]["labels"].shape[1] and g["dtype"] == x.dtype
        assert g["ld_out"] == gr.max_out(cfg, g["ld_lab"], chunk) and g["max_seg"] == gr.max_seg(cfg, g["ld_lab"])
        # the pool and the endpointer do not move
        for s in range(STEPS):
            assert np.array_equal(got[s]["counts"], plain[s]["counts"]) and np.array_equal(got[s]["lab_counts"], plain[s]["lab_counts"])
            assert np.array_equal(got[s]["ev_counts"], plain[s]["ev_counts"]) and np.array_equal(got[s]["active"], plain[s]["active"])
            for b in range(B):
                n, ne, nl = int(plain[s]["counts"][b]), min(int(plain[s]["ev_counts"][b]), plain[s]["events"].shape[1]), int(plain[s]["lab_counts"][b])
                assert got[s]["logits"][b, :n].tobytes() == plain[s]["logits"][b, :n].tobytes(), (graphs, s, b)
                assert got[s]["probs"][b, :n].tobytes() == plain[s]["probs"][b, :n].tobytes(), (graphs, s, b)
                assert got[s]["events"][b, :ne].tobytes() == plain[s]["events"][b, :ne].tobytes(), (graphs, s, b)
                assert got[s]["labels"][b, :nl].tobytes() == plain[s]["labels"][b, :nl].tobytes(), (graphs, s, b)
        # every step against the step rule, on the labels this very run emitted
        chunks = np.stack([xs[:, s * chunk:(s + 1) * chunk] for s in range(STEPS)])
        labels, lab_counts = np.stack([r["labels"] for r in got]), np.stack([r["lab_counts"] for r in got])
        ref, _ = gr.simulate(cfg, g["history"], chunks, labels, lab_counts, flags, g["ld_out"], g["max_seg"])
        seen = 0
        for s in range(STEPS):
            seg = got[s]["seg"].view(gr.SEG_DTYPE).reshape(B, -1)
            for b, (want_out, want_seg, want_count) in enumerate(ref[s]):
                assert got[s]["seg_counts"][b] == want_count == len(want_seg), (graphs, s, b)
                assert seg[b, :want_count].tobytes() == want_seg.tobytes(), (graphs, s, b, seg[b, :want_count], want_seg)
                used = int(want_seg["n_stored"].sum())
                assert got[s]["out"][b, :used].tobytes() == want_out[:used].tobytes(), (graphs, s, b)
                seen |= int(np.bitwise_or.reduce(want_seg["flags"])) if want_count else 0
        assert seen == gr.FIRST | gr.LAST                                   # neither LOST nor SHORT with the pool's own geometry
        # ended sessions: speech_cuts on the session's own finalised labels and PCM
        n_cuts = n_split = 0
        for b, s0, s1 in _sessions(flags):
            lab = np.concatenate([got[s]["labels"][b, :got[s]["lab_counts"][b]] for s in range(s0, s1 + 1)])
            pcm = x[b:b + 1, s0 * chunk:(s1 + 1) * chunk].contiguous()
            recs = []
            for s in range(s0, s1 + 1):
                off = 0
                for r in got[s]["seg"].view(gr.SEG_DTYPE).reshape(B, -1)[b, :got[s]["seg_counts"][b]]:
                    recs.append((r, got[s]["out"][b, off:off + int(r["n_stored"])]))
                    off += int(r["n_stored"])
            cuts = gr.assemble(recs)
            if len(lab) == 0:
                assert not cuts
                continue
            ct = rt.cuts_open(**dict(zip(KEYS, cfg)))
            _, batch, blen = rt.speech_cuts(torch.from_numpy(lab[None, :].copy()).to(DEV), pcm, cuts=ct)
            table, batch, blen = rt.cuts_read(ct), batch.cpu().numpy(), blen.cpu().numpy()
            assert len(cuts) == len(table), (graphs, b, s0, len(cuts), len(table))
            for i, (f, k, fl, samples, done) in enumerate(cuts):
                assert done and (f, k) == (table["first_frame"][i], table["n_frames"][i]) and table["index"][i] == i, (graphs, b, s0, i)
                assert len(samples) == table["n_samples"][i] == blen[i] and samples.tobytes() == batch[i, :len(samples)].tobytes(), (graphs, b, s0, i)
                n_split += k == cfg[1]
            n_cuts += len(cuts)
        print(f"graphs={graphs}: {n_cuts} cuts ({n_split} full pieces) over {int(lab_counts.sum())} labels, history {g['history']}")
        assert n_cuts > 0 and n_split > 0                                  # any interval here is longer than max_len = 3


def _thresholds(open_pool, step, x, chunk):
    """Percentiles of the probabilities the pool emits for this input, so that a model whose outputs sit on one side of 0.5 still gives
    labels on both sides."""
    plain, _ = _run(open_pool, step, x, _flags(), chunk, None, None, False)
    emitted = np.concatenate([rec["logits"][b, :int(rec["counts"][b])] for rec in plain for b in range(B)]).astype(np.float64)
    assert len(emitted) > 20
    sig = lambda z: float(np.float32(1.0 / (1.0 + np.exp(-z))))
    return [sig(np.percentile(emitted, p)) for p in (25, 40, 45)]


def test_logmel_pool_with_gate():
    chunk = 120                                                             # (frame_len - frame_shift) / 2: the smallest a log-mel pool takes
    m, rt = es._logmel_model()
    open_pool = lambda **kw: rt.window_slots_open(B, chunk, window=W, lookahead=L, **kw)
    x = _pcm(chunk, 31, torch.float32)
    lo, mid, hi = _thresholds(open_pool, rt.window_slots_step, x, chunk)
    geometry = (160, 120, 120)
    _check(rt, open_pool, rt.window_slots_step, x, chunk, {"kernel": 5, "pad": 2, "threshold": mid}, {"pad": 2, "max_len": 3}, geometry, 2)
    _check(rt, open_pool, rt.window_slots_step, x, chunk, dict(_INTS, onset=hi, offset=lo), {"max_len": 3}, geometry, 3 + 1 + 2 + 1)
    with pytest.raises(ValueError, match="gate needs an endpoint"):
        open_pool(gate={})
    with pytest.raises(ValueError):
        open_pool(endpoint={"kernel": 5}, gate={"taps": 3})
    with pytest.raises(ValueError):
        open_pool(endpoint={"kernel": 5}, gate={"min_len": 2})
    st = open_pool(endpoint={"kernel": 5}, gate={})                         # every default: the pool's geometry, pad 0, no splitting
    assert tuple(getattr(st["gate"]["cfg"], k) for k in KEYS) == (0, 0, 0) + geometry


def test_waveform_pool_with_gate():
    chunk = 270                                                             # one frame step
    m, rt = es._wav_model()
    open_pool = lambda **kw: rt.wav_window_slots_open(B, chunk, window=W, lookahead=L, dtype=torch.int16, **kw)
    x = _pcm(chunk, 32, torch.int16)
    lo, mid, hi = _thresholds(open_pool, rt.wav_window_slots_step, x, chunk)
    J, R = rt.wav_window_geometry()
    geometry = (J, 0, R - J)
    _check(rt, open_pool, rt.wav_window_slots_step, x, chunk, {"kernel": 5, "pad": 2, "threshold": mid}, {"pad": 2, "max_len": 3}, geometry, 2)
    _check(rt, open_pool, rt.wav_window_slots_step, x, chunk, dict(_INTS, onset=hi, offset=lo), {"max_len": 3}, geometry, 3 + 1 + 2 + 1)
    with pytest.raises(ValueError, match="gate needs an endpoint"):
        open_pool(gate={"max_len": 7})
