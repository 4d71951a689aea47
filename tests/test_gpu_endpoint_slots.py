"""GPU tests (-m gpu) of the endpointer behind both slot pools (window_slots_open / wav_window_slots_open with endpoint=...): the endpoint
step is enqueued right behind the pool step -- inside the one captured graph under graphs=True -- on the pool's probabilities, counts and
flags.  Its events, counts and active byte equal the reference applied to the probabilities the same run emitted, collected step by step,
and the pool's own outputs are byte-identical to a pool opened without an endpointer."""
import numpy as np
import pytest
import torch

import endpoint_ref as er

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_EP = {"kernel": 5, "pad": 2}
STEPS = 40


def _logmel_model(F=64, scale=2.0):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=F)
    m.build()
    seed_weights(m, 1234, scale)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type="povey"))
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


def _wav_model(seed=11, scale=2.0):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    torch.manual_seed(seed)
    m = uvad_amd.PyanNet()
    m.build()
    seed_weights(m, 1234, scale)
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


def _flags(B):
    """Staggered sessions: slot 0 from step 0, ended at 30; slot 1 from 4, restarted at 20 while busy, ended at 37; the last slot a
    one-step session at 6 and one from 9 that is still running when the schedule ends."""
    f = np.zeros((STEPS, B), np.uint8)
    f[0, 0], f[30, 0] = 1, 2
    f[4, 1], f[20, 1], f[37, 1] = 1, 1, 2
    f[6, B - 1], f[9, B - 1] = 3, 1
    return f


def _pcm(B, chunk, seed):
    """Bursts of noise and silence, a few chunks each, different per slot."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, STEPS * chunk), np.float32)
    for b in range(B):
        pos, loud = 0, bool(b % 2)
        while pos < x.shape[1]:
            n = int(rng.integers(2, 7)) * chunk
            if loud:
                x[b, pos:pos + n] = 0.3 * rng.standard_normal(min(n, x.shape[1] - pos)).astype(np.float32)
            pos, loud = pos + n, not loud
    return torch.from_numpy(x).to(DEV)


def _run(open_pool, step, x, flags, chunk, endpoint, graphs):
    st = open_pool(endpoint=endpoint, graphs=graphs)
    out = []
    for s in range(STEPS):
        fl = flags[s]
        xs = x[:, s * chunk:(s + 1) * chunk].contiguous()
        lg, cnt = step(st, xs, start=fl & 1 == 1, end=fl & 2 == 2) if fl.any() else step(st, xs)
        rec = {"logits": lg.clone(), "counts": cnt.clone()}
        if endpoint is not None:
            ep = st["endpoint"]
            rec.update(probs=st["probs"].clone(), **{k: ep[k].clone() for k in ("events", "ev_counts", "active", "labels", "lab_counts")})
        out.append(rec)
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in rec.items()} for rec in out], st


def _check(open_pool, step, x, flags, chunk, B, threshold=None):
    """threshold="low": the 30th percentile of the probabilities the pool emits for this input (taken from the run without an endpointer), so
    that a model whose outputs sit on one side of 0.5 still gives labels on both sides, most of them speech; None: the default 0.5."""
    plain, st0 = _run(open_pool, step, x, flags, chunk, None, False)
    assert "endpoint" not in st0 and "probs" not in st0
    EP = dict(_EP)
    if threshold == "low":
        emitted = np.concatenate([rec["logits"][b, :int(rec["counts"][b])] for rec in plain for b in range(B)])
        assert len(emitted) > 20
        EP["threshold"] = float(np.float32(1.0 / (1.0 + np.exp(-np.percentile(emitted.astype(np.float64), 30)))))
    thr = EP.get("threshold", 0.5)
    runs = {}
    for graphs in (False, True):
        got, st = _run(open_pool, step, x, flags, chunk, EP, graphs)
        runs[graphs] = got
        if graphs:
            assert st["graphs"] == 1                                        # pool step and endpoint step in the one capture
        ld = st["out"].shape[1]
        assert st["endpoint"]["ld_in"] == ld and st["endpoint"]["max_events"] == ld + EP["kernel"] // 2 + 2
        # the pool's own outputs do not move
        for s in range(STEPS):
            assert np.array_equal(got[s]["counts"], plain[s]["counts"]), (graphs, s)
            for b in range(B):
                n = int(plain[s]["counts"][b])
                assert got[s]["logits"][b, :n].tobytes() == plain[s]["logits"][b, :n].tobytes(), (graphs, s, b)
        # the endpointer on the probabilities this very run emitted
        counts = np.stack([g["counts"] for g in got])
        probs = np.stack([g["probs"] for g in got])
        for s in range(STEPS):
            for b in range(B):
                n = int(counts[s, b])
                assert np.allclose(probs[s, b, :n], 1.0 / (1.0 + np.exp(-got[s]["logits"][b, :n].astype(np.float64))), atol=1e-5)
        want = er.simulate(probs, counts, flags, EP["kernel"], EP["pad"], thr)
        n_events = 0
        for s, row in enumerate(want):
            for b, (y, ev, active) in enumerate(row):
                assert got[s]["ev_counts"][b] == len(ev), (graphs, s, b, ev)
                assert got[s]["events"][b, :len(ev)].tolist() == [list(e) for e in ev], (graphs, s, b)
                assert got[s]["active"][b] == active and got[s]["lab_counts"][b] == len(y), (graphs, s, b)
                assert np.array_equal(got[s]["labels"][b, :len(y)], y), (graphs, s, b)
                n_events += len(ev)
        # ended sessions: the whole-row answer
        for b, s0, s1, ended in er.sessions(counts, flags):
            if ended and flags[s0, b] & 1:
                row = er.session_row(probs, counts, b, s0, s1)
                evs = [tuple(e) for s in range(s0, s1 + 1) for e in got[s]["events"][b, :got[s]["ev_counts"][b]].tolist()]
                assert evs == er.events_of(er.whole(row, EP["kernel"], EP["pad"], thr)[1]), (graphs, b, s0)
        flips = sum(int(np.abs(np.diff(np.concatenate([got[s]["labels"][b, :got[s]["lab_counts"][b]] for s in range(STEPS)]).astype(np.int8))).sum())
                    for b in range(B))
        print(f"graphs={graphs}: threshold {thr:.6f}, {n_events} events, {flips} label changes over {int(counts.sum())} frames")
        assert n_events > 0
    return runs


def test_logmel_pool_with_endpoint():
    B, chunk, W, L = 3, 320, 50, 7
    m, rt = _logmel_model()
    _check(lambda **kw: rt.window_slots_open(B, chunk, window=W, lookahead=L, **kw), rt.window_slots_step, _pcm(B, chunk, 21), _flags(B), chunk, B)
    with pytest.raises(ValueError):
        rt.window_slots_open(B, chunk, window=W, lookahead=L, endpoint={"kernel": 4})
    with pytest.raises(ValueError):
        rt.window_slots_open(B, chunk, window=W, lookahead=L, endpoint={"taps": 5})


def test_waveform_pool_with_endpoint():
    B, chunk, W, L = 2, 320, 60, 7
    m, rt = _wav_model()
    _check(lambda **kw: rt.wav_window_slots_open(B, chunk, window=W, lookahead=L, **kw), rt.wav_window_slots_step, _pcm(B, chunk, 22), _flags(B),
           chunk, B, threshold="low")      # the seeded PyanNet's probabilities all lie below 0.5 on this input
