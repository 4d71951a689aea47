"""GPU tests (-m gpu) of the fusion node behind both slot pools (window_slots_open / wav_window_slots_open with fuse={"groups": ...}), at
the small pool shapes of tests/test_gpu_endpoint_hyst_slots.py (chunk 320, a few feeds), whose models and input are used as they are.
The slots are grouped in pairs and in threes and the START / END churn of tests/test_gpu_endpoint_slots.py is applied per group, so the
members of a group step in lockstep.  Run eager and as one graph:
  - the pool's own outputs are byte-identical to a pool opened without the node;
  - every step's fused rows, group counts, best positions and OR-ed flags equal tests/fuse_ref.py on the probabilities, counts and flags
    the same step emitted; the probability buffer is NaN before the first step and the fused buffer holds a canary, so an idle group that
    was read, or written, shows;
  - the hysteresis endpointer, opened for the groups, equals the frame-loop simulator on the fused rows, and for every ended session the
    concatenated events and labels are byte-identical to uvad_binarize on the offline fusion (uvad_fuse on the members' whole sessions);
  - the counters accumulated over the session equal the sum of the steps' references."""
import numpy as np
import pytest
import torch

import binarize_ref as br
import endpoint_hyst_ref as hr
import endpoint_ref as er
import fuse_ref as fr
import test_gpu_endpoint_slots as es

pytestmark = pytest.mark.gpu

STEPS = es.STEPS
_INTS = {"min_on": 3, "min_off": 2, "pad_on": 1, "pad_off": 2}
CANARY = -77.0


def _run(open_pool, step, x, flags, chunk, fuse, endpoint, graphs):
    st = open_pool(fuse=fuse, endpoint=endpoint, graphs=graphs)
    if fuse is not None:
        st["probs"].fill_(float("nan"))
        st["fuse"]["fused"].fill_(CANARY)
    out = []
    for s in range(STEPS):
        fl = flags[s]
        xs = x[:, s * chunk:(s + 1) * chunk].contiguous()
        lg, cnt = step(st, xs, start=fl & 1 == 1, end=fl & 2 == 2) if fl.any() else step(st, xs)
        rec = {"logits": lg.clone(), "counts": cnt.clone()}
        if fuse is not None:
            fz, ep = st["fuse"], st["endpoint"]
            rec.update(probs=st["probs"].clone(), fused=fz["fused"].clone(), glens=fz["glens"].clone(), best=fz["best"].clone(),
                       gflags=fz["flags"].clone(), **{k: ep[k].clone() for k in ("events", "ev_counts", "active", "labels", "lab_counts")})
            fz["fused"].fill_(CANARY)
        out.append(rec)
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in rec.items()} for rec in out], st


def _check(rt, open_pool, step, x, B, chunk, groups, mode):
    G = len(groups)
    gflags = es._flags(G)
    flags = np.zeros((STEPS, B), np.uint8)
    for g, rows in enumerate(groups):
        flags[:, rows] = gflags[:, g:g + 1]
    plain, st0 = _run(open_pool, step, x, flags, chunk, None, None, False)
    assert "fuse" not in st0 and "probs" not in st0
    emitted = np.concatenate([rec["logits"][b, :int(rec["counts"][b])] for rec in plain for b in range(B)]).astype(np.float64)
    assert len(emitted) > 20
    sig = lambda z: float(np.float32(1.0 / (1.0 + np.exp(-z))))
    EP = dict(_INTS, onset=sig(np.percentile(emitted, 60)), offset=sig(np.percentile(emitted, 40)))
    assert EP["offset"] < EP["onset"]
    q = br.cfg(**EP)
    FZ = {"groups": groups, "mode": mode, "threshold": EP["onset"]}
    m = {"max": fr.MAX, "mean": fr.MEAN, "vote": fr.VOTE}[mode]
    dec = 0.5 if mode == "vote" else EP["onset"]
    for graphs in (False, True):
        got, st = _run(open_pool, step, x, flags, chunk, FZ, EP, graphs)
        if graphs:
            assert st["graphs"] == 1                                        # pool step, fusion and endpoint step in the one capture
        ld, ep, fz = st["out"].shape[1], st["endpoint"], st["fuse"]
        assert ep["B"] == G and ep["ld_in"] == ld and tuple(fz["fused"].shape) == (G, ld)
        total = np.zeros((B, 4), np.uint64)
        for s in range(STEPS):
            assert np.array_equal(got[s]["counts"], plain[s]["counts"]), (graphs, s)       # the pool's own outputs do not move
            for b in range(B):
                n = int(plain[s]["counts"][b])
                assert got[s]["logits"][b, :n].tobytes() == plain[s]["logits"][b, :n].tobytes(), (graphs, s, b)
            for rows in groups:                                                             # lockstep: what the node is specified for
                assert len({int(got[s]["counts"][r]) for r in rows}) == 1
            ref = fr.fuse_ref(got[s]["probs"], groups, m, EP["onset"], dec, got[s]["counts"], flags=flags[s] if graphs or flags[s].any() else None)
            assert got[s]["glens"].tolist() == ref["glens"].tolist(), (graphs, s)
            for g in range(G):
                L = int(ref["glens"][g])
                assert got[s]["fused"][g, :L].tobytes() == ref["fused"][g, :L].tobytes(), (graphs, s, g)
                assert (got[s]["fused"][g, L:] == CANARY).all(), (graphs, s, g)             # an idle group's row is not written at all
                assert got[s]["best"][g, :L].tobytes() == ref["best"][g, :L].tobytes(), (graphs, s, g)
                assert not np.isnan(got[s]["fused"][g, :L]).any()                           # nothing past a count, no idle row was read
            if "flags" in ref:
                assert got[s]["gflags"].tolist() == ref["flags"].tolist() == gflags[s].tolist(), (graphs, s)
            total += ref["stats"]
        assert fz["stats"].cpu().numpy().view(np.uint64).tobytes() == total.tobytes()
        read = rt.fuse_read(fz)                                                              # per group, members in slot order
        assert [len(grp) for grp in read] == [len(rows) for rows in groups]
        assert [[d["valid"], d["speech"], d["agree"], d["best"]] for grp in read for d in grp] == total.tolist()
        # the endpointer on the fused rows this very run emitted
        counts = np.stack([g_["glens"] for g_ in got])
        probs = np.stack([g_["fused"] for g_ in got])
        want = hr.simulate(probs, counts, gflags, q)
        n_events = 0
        for s, row in enumerate(want):
            for g, (y, ev, active) in enumerate(row):
                assert got[s]["ev_counts"][g] == len(ev), (graphs, s, g, ev)
                assert got[s]["events"][g, :len(ev)].tolist() == [list(e) for e in ev], (graphs, s, g)
                assert got[s]["active"][g] == active and got[s]["lab_counts"][g] == len(y), (graphs, s, g)
                assert np.array_equal(got[s]["labels"][g, :len(y)], y), (graphs, s, g)
                n_events += len(ev)
        assert n_events > 0
        # ended sessions: uvad_binarize on the offline fusion of the members' whole sessions
        member_counts = np.stack([g_["counts"] for g_ in got])
        member_probs = np.stack([g_["probs"] for g_ in got])
        ended = 0
        for g, s0, s1, done in er.sessions(counts, gflags):
            if not (done and gflags[s0, g] & 1):
                continue
            rows = np.stack([er.session_row(member_probs, member_counts, r, s0, s1) for r in groups[g]])
            if rows.shape[1] == 0:                                                          # a session too short for a frame: nothing to fuse
                assert sum(int(got[s]["ev_counts"][g]) + int(got[s]["lab_counts"][g]) for s in range(s0, s1 + 1)) == 0
                continue
            off = rt.fuse_open([list(range(len(rows)))], mode=mode, threshold=EP["onset"])
            fused, glens, _, _, _ = rt.fuse(torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(es.DEV), state=off)
            lab, iv, cnt = rt.binarize(fused, lengths=glens, **EP)
            n = rows.shape[1]
            evs = [tuple(e) for s in range(s0, s1 + 1) for e in got[s]["events"][g, :got[s]["ev_counts"][g]].tolist()]
            labs = np.concatenate([got[s]["labels"][g, :got[s]["lab_counts"][g]] for s in range(s0, s1 + 1)])
            ivs = [tuple(v) for v in iv[0, :int(cnt.cpu()[0])].cpu().tolist()]
            assert int(glens.cpu()[0]) == n and labs.tobytes() == lab[0, :n].cpu().numpy().tobytes(), (graphs, g, s0)
            assert evs == hr.events_of(ivs), (graphs, g, s0)
            ended += 1
        assert ended > 0


def _refusals(open_pool, B):
    with pytest.raises(ValueError, match="gate"):
        open_pool(fuse={"groups": [[0, 1]]}, endpoint={"onset": 0.5}, gate={})
    for bad in ({"mode": "max"}, {"groups": [[0, B]]}, {"groups": [[]]}, {"groups": [[0, 1]], "mode": "median"},
                {"groups": [[0, 1]], "weights": [[0.0, 0.0]]}, {"groups": [[0, 1]], "threshold": float("nan")}):
        with pytest.raises(ValueError):
            open_pool(fuse=bad)


def test_logmel_pool_with_fusion():
    B, chunk, W, L = 6, 320, 50, 7
    m, rt = es._logmel_model()
    open_pool = lambda **kw: rt.window_slots_open(B, chunk, window=W, lookahead=L, **kw)
    x = es._pcm(B, chunk, 21)
    _check(rt, open_pool, rt.window_slots_step, x, B, chunk, [[0, 1], [2, 3], [4, 5]], "max")
    _check(rt, open_pool, rt.window_slots_step, x, B, chunk, [[0, 2, 4], [1, 3, 5]], "mean")
    _refusals(open_pool, B)


def test_waveform_pool_with_fusion():
    B, chunk, W, L = 6, 320, 60, 7
    m, rt = es._wav_model()
    open_pool = lambda **kw: rt.wav_window_slots_open(B, chunk, window=W, lookahead=L, **kw)
    x = es._pcm(B, chunk, 22)
    _check(rt, open_pool, rt.wav_window_slots_step, x, B, chunk, [[0, 1], [2, 3], [4, 5]], "vote")
    _check(rt, open_pool, rt.wav_window_slots_step, x, B, chunk, [[0, 1, 2], [3, 4, 5]], "max")
    _refusals(open_pool, B)
