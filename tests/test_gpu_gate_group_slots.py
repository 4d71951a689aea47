"""GPU tests (-m gpu) of the group gate behind both slot pools (window_slots_open / wav_window_slots_open with fuse=, endpoint= and
group_gate=), at the small pool shapes of tests/test_gpu_fuse_slots.py (chunk 320, six feeds in pairs and in threes, the per-group START /
END churn of tests/test_gpu_endpoint_slots.py).  Run eager and as one graph:
  - the pool's, the fusion's and the endpointer's outputs are byte-identical to the same pool opened without group_gate;
  - every step's records and fragments equal tests/gate_group_ref.py on the best bytes, labels and flags this very run emitted, and no
    record is LOST, SHORT or UNSYNC with the pool's own geometry and the derived histories;
  - every ended session's fragments, concatenated per cut, equal the offline device chain on that session: uvad_fuse on the members'
    whole probabilities, uvad_binarize, uvad_cuts_table, uvad_fuse_pick, uvad_cuts_gather on the members' audio (D >= max_len)."""
import numpy as np
import pytest
import torch

import endpoint_ref as er
import gate_group_ref as gg
import test_gpu_endpoint_slots as es

pytestmark = pytest.mark.gpu

STEPS = es.STEPS
_INTS = {"min_on": 3, "min_off": 2, "pad_on": 1, "pad_off": 2}
KEYS = ("pad", "max_len", "min_len", "hop", "lead", "tail")
FZ_OUT = ("fused", "glens", "best", "flags")
EP_OUT = ("events", "ev_counts", "active", "labels", "lab_counts")
GG_OUT = ("out", "seg", "seg_counts")


def _run(open_pool, step, x, flags, chunk, fuse, endpoint, group_gate, graphs):
    st = open_pool(fuse=fuse, endpoint=endpoint, group_gate=group_gate, graphs=graphs)
    out = []
    for s in range(STEPS):
        fl = flags[s]
        xs = x[:, s * chunk:(s + 1) * chunk].contiguous()
        lg, cnt = step(st, xs, start=fl & 1 == 1, end=fl & 2 == 2) if fl.any() else step(st, xs)
        rec = {"logits": lg.clone(), "counts": cnt.clone()}
        if fuse is not None:
            rec.update(probs=st["probs"].clone(), **{k: st["fuse"][k].clone() for k in FZ_OUT}, **{k: st["endpoint"][k].clone() for k in EP_OUT})
        if group_gate is not None:
            rec.update({k: st["group_gate"][k].clone() for k in GG_OUT})
        out.append(rec)
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in rec.items()} for rec in out], st


def _check(rt, open_pool, step, x, B, chunk, groups, geometry, D, max_len):
    G = len(groups)
    gflags = es._flags(G)
    flags = np.zeros((STEPS, B), np.uint8)
    for g, rows in enumerate(groups):
        flags[:, rows] = gflags[:, g:g + 1]
    bare, _ = _run(open_pool, step, x, flags, chunk, None, None, None, False)
    emitted = np.concatenate([rec["logits"][b, :int(rec["counts"][b])] for rec in bare for b in range(B)]).astype(np.float64)
    sig = lambda z: float(np.float32(1.0 / (1.0 + np.exp(-z))))
    EP = dict(_INTS, onset=sig(np.percentile(emitted, 60)), offset=sig(np.percentile(emitted, 40)))
    FZ = {"groups": groups, "mode": "max", "threshold": EP["onset"]}
    GATE = {"decide_frames": D, "max_len": max_len}
    hop, lead, tail = geometry
    cfg = (0, max_len, 0, hop, lead, tail)
    xs = x.cpu().numpy()
    for graphs in (False, True):
        plain, st0 = _run(open_pool, step, x, flags, chunk, FZ, EP, None, graphs)
        got, st = _run(open_pool, step, x, flags, chunk, FZ, EP, GATE, graphs)
        assert "group_gate" not in st0 and "gate" not in st
        if graphs:
            assert st["graphs"] == 1                                        # pool step, fusion, endpoint step and group gate in the one capture
        gt, ep = st["group_gate"], st["endpoint"]
        lag = st["lookahead"] + ep["lag"] + -(-tail // hop)
        assert tuple(getattr(gt["cfg"], k) for k in KEYS) == cfg and gt["lag_frames"] == lag and gt["decide_frames"] == D
        assert gt["history"] == gg.history(cfg, lag, chunk, D) and gt["best_history"] == gg.best_history(cfg, lag, chunk, D)
        assert gt["ld_lab"] == ep["labels"].shape[1] and gt["dtype"] == x.dtype and gt["G"] == G
        assert gt["ld_out"] == gg.max_out(cfg, gt["ld_lab"], chunk, D) and gt["max_seg"] == gg.max_seg(cfg, gt["ld_lab"])
        # the pool, the fusion and the endpointer do not move
        for s in range(STEPS):
            for k in ("counts", "glens", "flags", "ev_counts", "active", "lab_counts"):
                assert np.array_equal(got[s][k], plain[s][k]), (graphs, s, k)
            for b in range(B):
                n = int(plain[s]["counts"][b])
                assert got[s]["logits"][b, :n].tobytes() == plain[s]["logits"][b, :n].tobytes(), (graphs, s, b)
                assert got[s]["probs"][b, :n].tobytes() == plain[s]["probs"][b, :n].tobytes(), (graphs, s, b)
            for g in range(G):
                n, ne, nl = int(plain[s]["glens"][g]), min(int(plain[s]["ev_counts"][g]), plain[s]["events"].shape[1]), int(plain[s]["lab_counts"][g])
                assert got[s]["fused"][g, :n].tobytes() == plain[s]["fused"][g, :n].tobytes(), (graphs, s, g)
                assert got[s]["best"][g, :n].tobytes() == plain[s]["best"][g, :n].tobytes(), (graphs, s, g)
                assert got[s]["events"][g, :ne].tobytes() == plain[s]["events"][g, :ne].tobytes(), (graphs, s, g)
                assert got[s]["labels"][g, :nl].tobytes() == plain[s]["labels"][g, :nl].tobytes(), (graphs, s, g)
        # every step against the step rule, on what this very run emitted
        grp = [gg.Group(cfg, len(rows), gt["history"], gt["best_history"], D, xs.dtype) for rows in groups]
        seen, res = 0, [[] for _ in range(G)]
        for s in range(STEPS):
            seg = got[s]["seg"].view(gg.SEG_DTYPE).reshape(G, -1)
            for g, rows in enumerate(groups):
                live = grp[g].live or gflags[s, g] & 1
                want_out, want_seg, want_count = grp[g].step(
                    xs[rows, s * chunk:(s + 1) * chunk], got[s]["best"][g, :got[s]["glens"][g]] if live else (),
                    got[s]["labels"][g, :got[s]["lab_counts"][g]] if live else (), int(gflags[s, g]), gt["ld_out"], gt["max_seg"])
                assert got[s]["seg_counts"][g] == want_count == len(want_seg), (graphs, s, g)
                assert seg[g, :want_count].tobytes() == want_seg.tobytes(), (graphs, s, g, seg[g, :want_count], want_seg)
                used = int(want_seg["n_stored"].sum())
                assert got[s]["out"][g, :used].tobytes() == want_out[:used].tobytes(), (graphs, s, g)
                seen |= int(np.bitwise_or.reduce(want_seg["flags"])) & 0xff if want_count else 0
                res[g].append((got[s]["out"][g], seg[g, :want_count], want_count))
        assert seen == gg.FIRST | gg.LAST and all(p.voteless == 0 for p in grp)
        # ended sessions: the offline device chain on the members' whole sessions
        counts = np.stack([r["glens"] for r in got])
        member_counts, member_probs = np.stack([r["counts"] for r in got]), np.stack([r["probs"] for r in got])
        n_cuts = n_sessions = 0
        picked = set()
        for g, s0, s1, done in er.sessions(counts, gflags):
            if not (done and gflags[s0, g] & 1):
                continue
            cuts = gg.session_cuts(res[g][s0:s1 + 1])
            rows = np.stack([er.session_row(member_probs, member_counts, r, s0, s1) for r in groups[g]])
            if rows.shape[1] == 0:
                assert not cuts
                continue
            S = (s1 + 1 - s0) * chunk
            off = rt.fuse_open([list(range(len(rows)))], mode="max", threshold=EP["onset"])
            fused, glens, _, best, _ = rt.fuse(torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(es.DEV), state=off)
            lab, _, _ = rt.binarize(fused, lengths=glens, **EP)
            ct = rt.cuts_open(**dict(zip(KEYS, cfg)))
            rt.cuts_table(lab, lengths=glens, S=S, cuts=ct)
            ptab, pick = rt.fuse_pick(best, ct, state=off)
            pcm = x[groups[g], s0 * chunk:(s1 + 1) * chunk].contiguous()
            batch, blen = rt.cuts_gather(pcm, ct, "samples", table=ptab)
            tab, batch, blen, pick = rt.cuts_read(ct), batch.cpu().numpy(), blen.cpu().numpy(), pick.cpu().numpy()
            assert len(cuts) == len(tab), (graphs, g, s0, len(cuts), len(tab))
            for i, (f, k, fl, data, fin) in enumerate(cuts):
                assert fin and (f, k, gg.channel(fl)) == (int(tab[i]["first_frame"]), int(tab[i]["n_frames"]), int(pick[i])), (graphs, g, s0, i)
                assert len(data) == blen[i] == tab[i]["n_samples"] and data.tobytes() == batch[i, :blen[i]].tobytes(), (graphs, g, s0, i)
                picked.add(gg.channel(fl))
            n_cuts += len(cuts)
            n_sessions += 1
        print(f"graphs={graphs} groups={groups}: {n_sessions} ended sessions, {n_cuts} cuts, channels {sorted(picked)}, history {gt['history']} / "
              f"{gt['best_history']}, state {gt['state'].numel()} bytes")
        assert n_sessions > 0 and n_cuts > 0
        recs = rt.gate_group_collect(gt)                                     # the host view of the last step
        assert [len(r) for r in recs] == [int(c) for c in got[-1]["seg_counts"]]


def _refusals(open_pool):
    with pytest.raises(ValueError, match="gate= together with fuse= is not built"):
        open_pool(fuse={"groups": [[0, 1]]}, endpoint={"onset": 0.5}, gate={})
    with pytest.raises(ValueError, match="group_gate needs fuse= and endpoint="):
        open_pool(fuse={"groups": [[0, 1]]}, group_gate={"decide_frames": 3})
    with pytest.raises(ValueError, match="group_gate needs fuse= and endpoint="):
        open_pool(endpoint={"onset": 0.5}, group_gate={"decide_frames": 3})
    with pytest.raises(ValueError, match="decide_frames"):
        open_pool(fuse={"groups": [[0, 1]]}, endpoint={"onset": 0.5}, group_gate={"max_len": 3})


def test_logmel_pool_with_group_gate():
    B, chunk, W, L = 6, 320, 50, 7
    m, rt = es._logmel_model()
    open_pool = lambda **kw: rt.window_slots_open(B, chunk, window=W, lookahead=L, **kw)
    x = es._pcm(B, chunk, 21)
    _check(rt, open_pool, rt.window_slots_step, x, B, chunk, [[0, 1], [2, 3], [4, 5]], (160, 120, 120), 5, 5)
    _check(rt, open_pool, rt.window_slots_step, x, B, chunk, [[0, 2, 4], [1, 3, 5]], (160, 120, 120), 25, 6)
    _refusals(open_pool)


def test_waveform_pool_with_group_gate():
    B, chunk, W, L = 6, 320, 60, 7
    m, rt = es._wav_model()
    open_pool = lambda **kw: rt.wav_window_slots_open(B, chunk, window=W, lookahead=L, **kw)
    x = es._pcm(B, chunk, 22)
    J, R = rt.wav_window_geometry()
    _check(rt, open_pool, rt.wav_window_slots_step, x, B, chunk, [[0, 1], [2, 3], [4, 5]], (J, 0, R - J), 4, 4)
    _check(rt, open_pool, rt.wav_window_slots_step, x, B, chunk, [[0, 1, 2], [3, 4, 5]], (J, 0, R - J), 1000, 7)
    _refusals(open_pool)
