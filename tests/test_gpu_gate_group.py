"""GPU tests (-m gpu) of the group gate (uvad_gate_group_*, include/uvad.h) through VadRuntime.gate_group_open / gate_group_step on a
post-processing context: every step's out / seg / seg_counts bytes against the step rule restated in tests/gate_group_ref.py (the buffers
are filled with a canary before every step: nothing is written beside the records and fragments); ended sessions against the device chain
uvad_fuse -> uvad_cuts_table -> uvad_fuse_pick -> uvad_cuts_gather at D >= max_len and against the numpy definition at D = 1 and 3; the
hand-made cases; NaN and junk wherever nothing may be read; max_seg and ld_out overflow; the rings at their bound and below it; UNSYNC;
determinism; one captured graph replayed for every later step; one-member groups at D = 1 against the mono gate on the device; and the
refusals that need a reset state.  hop 4, lead 3, tail 3, sessions
of at most 120 frames, G = 4 groups over B = 8 rows: one member, two, three (sharing a row with the pair) and 70."""
import ctypes as C

import numpy as np
import pytest
import torch

import fuse_ref as fr
import gate_group_ref as gg
import gate_ref as gr
import test_gate_group_ref as tr
import test_gate_ref as tg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY = 0x5A
E_ARG, E_STATE = -1, -3
HOP, LEAD, TAIL = tr.HOP, tr.LEAD, tr.TAIL
KEYS = ("pad", "max_len", "min_len", "hop", "lead", "tail")
B = 8
GROUPS = [[3], [0, 1], [2, 5, 1], [(5 * i + 2) % 7 for i in range(70)]]     # row 7 is in no group
TORCH = {np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32}


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def _probs(rng, M, n):
    """(M, n) member probabilities: a shared pattern of runs, each member hearing it at its own level."""
    base = np.full(n, 0.2, np.float32)
    t = int(rng.integers(0, 6))
    while t < n:
        run = int(rng.integers(1, 22))
        base[t:t + run] = 0.7
        t += run + int(rng.integers(1, 14))
    lvl = np.repeat(rng.uniform(-0.15, 0.25, (M, n // 3 + 1)), 3, axis=1)[:, :n]
    return (base[None, :] + lvl).astype(np.float32)


def random_sessions(rng, groups, chunk, steps, way):
    """Per group a list of sessions {s0, len, probs, labels, best, way}: back to back or with idle steps between them, every one ended."""
    out = []
    longest = max(1, (120 * HOP + TAIL) // chunk)
    for rows in groups:
        mine, s = [], int(rng.integers(0, 3))
        while s < steps:
            n_steps = min(int(rng.integers(1, longest + 1)), steps - s)
            n = max(0, (n_steps * chunk - TAIL) // HOP)
            p = _probs(rng, len(rows), n)
            ref = fr.fuse_ref(p, [list(range(len(rows)))], fr.MAX, 0.5, 0.5) if n else {"labels": np.zeros((1, 0), np.uint8), "best": np.zeros((1, 0), np.uint8)}
            mine.append({"s0": s, "len": n_steps, "probs": p, "labels": ref["labels"][0], "best": ref["best"][0], "way": way})
            s += n_steps + int(rng.integers(0, 3))
        out.append(mine)
    return out


def make_script(groups, chunk, dtype, steps, sessions, lag, seed, rflags=None):
    """The per-step device inputs: x (B, steps chunk) the rows' samples (row 7, which no group names, is NaN where the type has one);
    best / labels with their counts and the group flags, with junk in every column past a count and in everything of an idle group."""
    rng = np.random.default_rng(seed)
    G = len(groups)
    if np.dtype(dtype) == np.int16:
        x = rng.integers(-30000, 30000, (B, steps * chunk)).astype(np.int16)
    else:
        x = rng.standard_normal((B, steps * chunk)).astype(np.float32)
        x[7] = np.nan
    plan = [[None] * G for _ in range(steps)]
    for g, mine in enumerate(sessions):
        for ses in mine:
            S, n = ses["len"] * chunk, len(ses["labels"])
            front = [(0, 0)] + tr._frontier(ses["way"], rng, S, n, chunk, lag)
            for i in range(ses["len"]):
                fl = (gg.START if i == 0 else 0) | (gg.END if i == ses["len"] - 1 else 0)
                assert plan[ses["s0"] + i][g] is None
                plan[ses["s0"] + i][g] = (ses["labels"][front[i][0]:front[i + 1][0]], ses["best"][front[i][1]:front[i + 1][1]], fl)
    ld_lab = max([len(p[0]) for row in plan for p in row if p] + [1]) + 3
    ld_best = max([len(p[1]) for row in plan for p in row if p] + [1]) + 3
    labels, best = rng.integers(0, 256, (steps, G, ld_lab)).astype(np.uint8), rng.integers(0, 256, (steps, G, ld_best)).astype(np.uint8)
    lab_counts = rng.choice(np.array([-5, 3, 1 << 20], np.int32), (steps, G))
    best_counts = rng.choice(np.array([-9, 2, 1 << 21], np.int32), (steps, G))
    gflags = np.zeros((steps, G), np.uint8)
    for s in range(steps):
        for g in range(G):
            if plan[s][g]:
                lab, bst, fl = plan[s][g]
                labels[s, g, :len(lab)] = lab * rng.integers(1, 256, len(lab)).astype(np.uint8) if len(lab) else lab   # any non-zero byte is speech
                best[s, g, :len(bst)] = bst
                lab_counts[s, g], best_counts[s, g], gflags[s, g] = len(lab), len(bst), fl
    rf = np.zeros((steps, B), np.uint8) if rflags is None else rflags
    return {"groups": groups, "chunk": chunk, "steps": steps, "x": x, "plan": plan, "labels": labels, "best": best, "lab_counts": lab_counts,
            "best_counts": best_counts, "gflags": gflags, "rflags": rf, "sessions": sessions, "ld_lab": ld_lab, "ld_best": ld_best}


def reference(sc, cfg, D, hist, bh, ld_out, max_seg):
    grp = [gg.Group(cfg, len(rows), hist, bh, D, sc["x"].dtype) for rows in sc["groups"]]
    c, res = sc["chunk"], []
    for s in range(sc["steps"]):
        row = []
        for g, rows in enumerate(sc["groups"]):
            p = sc["plan"][s][g]
            lab, bst, fl = p if p else ((), (), 0)
            differ = len({int(sc["rflags"][s, r]) for r in rows}) > 1
            row.append(grp[g].step(sc["x"][rows, s * c:(s + 1) * c], bst, lab, fl, ld_out, max_seg, differ))
        res.append(row)
    return res, grp


def device_run(rt, sc, cfg, D, hist, bh, ld_out, max_seg, graph_at=None, rflags=True):
    """Every step through gate_group_step (from step graph_at on: one graph captured there and replayed) -> [(out, seg, seg_counts)] as
    numpy, out and seg pre-filled with the canary before every step."""
    G, c = len(sc["groups"]), sc["chunk"]
    fz = rt.fuse_open(sc["groups"])
    g = rt.gate_group_open(fz, c, sc["ld_lab"], TORCH[sc["x"].dtype], 0, D, history=hist, best_history=bh, ld_out=ld_out, max_seg=max_seg,
                           **dict(zip(KEYS, cfg)))
    assert g["history"] == hist and g["best_history"] == bh and g["out"].shape == (G, max(ld_out, 1)) and g["seg"].shape == (G, max(max_seg, 1), 8)
    assert g["state"].numel() == gg.state_bytes(G, sum(len(r) for r in sc["groups"]), sc["x"].dtype.itemsize, hist, bh)
    x = torch.from_numpy(np.ascontiguousarray(sc["x"].reshape(B, sc["steps"], c).transpose(1, 0, 2))).to(DEV)
    dev = {k: torch.from_numpy(sc[k]).to(DEV) for k in ("labels", "best", "lab_counts", "best_counts", "gflags", "rflags")}
    dev["x"] = x
    st = {k: torch.empty_like(v[0]) for k, v in dev.items()}
    graph, got = None, []
    for s in range(sc["steps"]):
        g["out"].view(torch.uint8).fill_(CANARY)
        g["seg"].view(torch.uint8).fill_(CANARY)
        g["seg_counts"].fill_(-7)
        if graph_at is None or s < graph_at:
            fl = dev["gflags"][s]
            rt.gate_group_step(g, x[s], dev["best"][s], dev["best_counts"][s], dev["labels"][s], dev["lab_counts"][s], start=(fl & 1).bool(),
                               end=(fl & 2).bool(), row_flags=dev["rflags"][s] if rflags else None)
        else:
            for k, v in dev.items():
                st[k].copy_(v[s])
            if graph is None:
                cur = torch.cuda.current_stream(DEV)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):                               # capture: recorded, not run
                    r = rt._gate_group_enqueue(g, st["x"].data_ptr(), B, st["best"].data_ptr(), sc["ld_best"], st["best_counts"].data_ptr(),
                                               st["labels"].data_ptr(), st["lab_counts"].data_ptr(), st["gflags"].data_ptr(),
                                               st["rflags"].data_ptr() if rflags else None)
                assert r == 0
                torch.cuda.current_stream(DEV).wait_stream(cur)
            graph.replay()
        got.append((g["out"].clone(), g["seg"].clone(), g["seg_counts"].clone()))
    torch.cuda.synchronize()
    return [(o.cpu().numpy(), sg.cpu().numpy().view(gg.SEG_DTYPE).reshape(G, -1), n.cpu().numpy()) for o, sg, n in got], g


def compare(got, ref, ld_out, max_seg):
    """Bytes of every step and group; what lies behind the records and the fragments still holds the canary."""
    n_rec = n_units = flags = 0
    for s, ((out, seg, counts), row) in enumerate(zip(got, ref)):
        for g, (want_out, want_seg, want_count) in enumerate(row):
            assert counts[g] == want_count, (s, g, counts[g], want_count)
            k = len(want_seg)
            assert k == min(want_count, max_seg)
            assert seg[g, :k].tobytes() == want_seg.tobytes(), (s, g, seg[g, :k], want_seg)
            assert (seg[g, k:].view(np.uint8) == CANARY).all(), (s, g)
            used = int(want_seg["n_stored"].sum())
            assert used <= ld_out and out[g, :used].tobytes() == want_out[:used].tobytes(), (s, g)
            assert (out[g, used:].view(np.uint8) == CANARY).all(), (s, g)
            n_rec += k
            n_units += used
            for f in want_seg["flags"]:
                flags |= int(f) & 0xff
    return n_rec, n_units, flags


def device_cuts(got, g, ses):
    """The fragments one session emitted on the device, assembled per cut."""
    res = [(got[s][0][g], got[s][1][g, :got[s][2][g]], int(got[s][2][g])) for s in range(ses["s0"], ses["s0"] + ses["len"])]
    return gg.session_cuts(res)


_CASES = {}


def case(chunk, dtype, way, cfg, D, seed, steps, extra_lag=5, hist=None, bh=None, ld_out=None, max_seg=None, groups=None, rflags=None):
    """The inputs and the restatement's answer, computed once per case and shared."""
    key = (chunk, np.dtype(dtype).str, way, cfg, D, seed, steps, extra_lag, hist, bh, ld_out, max_seg, None if groups is None else len(groups[0]),
           None if rflags is None else rflags.tobytes())
    if key not in _CASES:
        groups = GROUPS if groups is None else groups
        lag = tr.LAG0 + (0 if way in ("prompt", "big", "one") else extra_lag)
        rng = np.random.default_rng(seed)
        sc = make_script(groups, chunk, dtype, steps, random_sessions(rng, groups, chunk, steps, way), lag, seed + 1, rflags)
        h = gg.history(cfg, lag, chunk, D) if hist is None else hist
        b = gg.best_history(cfg, lag, chunk, D) if bh is None else bh
        lo = gg.max_out(cfg, sc["ld_lab"], chunk, D) if ld_out is None else ld_out
        ms = gg.max_seg(cfg, sc["ld_lab"]) if max_seg is None else max_seg
        ref, grp = reference(sc, cfg, D, h, b, lo, ms)
        _CASES[key] = (sc, ref, grp, h, b, lo, ms, lag)
    return _CASES[key]


CFG = (2, 7, 0, HOP, LEAD, TAIL)


@pytest.mark.parametrize("chunk,dtype,way,D,steps", [(6, np.int16, "prompt", 3, 90), (6, np.float32, "lagged", 7, 90), (6, np.int16, "bursts", 1, 90),
                                                     (24, np.float32, "big", 3, 40), (24, np.int16, "big", 1000, 40), (400, np.int16, "one", 7, 8),
                                                     (400, np.float32, "one", 1, 8)])
def test_every_step_equals_the_restatement(rt, chunk, dtype, way, D, steps):
    sc, ref, grp, h, b, lo, ms, lag = case(chunk, dtype, way, CFG, D, 31, steps)
    got, g = device_run(rt, sc, CFG, D, h, b, lo, ms)
    q = C.byref(g["cfg"])
    assert h == rt.lib.uvad_gate_group_history(q, lag, chunk, D) and b == rt.lib.uvad_gate_group_best_history(q, lag, chunk, D)
    assert lo == rt.lib.uvad_gate_group_max_out(q, sc["ld_lab"], chunk, D)
    n_rec, n_units, flags = compare(got, ref, lo, ms)
    print(f"chunk {chunk} {np.dtype(dtype).name} {way} D {D}: {len(got)} steps, {n_rec} records, {n_units} samples, history {h} / {b}, "
          f"state {g['state'].numel()} bytes")
    assert n_rec > 20 and flags == gg.FIRST | gg.LAST                       # neither LOST nor SHORT nor UNSYNC at the derived sizes
    assert chunk == 400 or h % chunk != 0                                   # rings whose length is no multiple of the chunk
    assert all(p.voteless == 0 for p in grp)
    # every ended session against the numpy definition
    n_cuts = 0
    for gi, mine in enumerate(sc["sessions"]):
        rows = sc["groups"][gi]
        for ses in mine:
            audio = sc["x"][rows, ses["s0"] * chunk:(ses["s0"] + ses["len"]) * chunk]
            want = gg.offline(ses["labels"], ses["best"], audio, CFG, D)
            cuts = device_cuts(got, gi, ses)
            assert [(f, k, gg.channel(fl), d.tobytes()) for f, k, fl, d, _ in cuts] == [(f, k, p, d.tobytes()) for f, k, p, d in want], (gi, ses["s0"])
            n_cuts += len(cuts)
    assert n_cuts > 8


def test_ended_sessions_equal_the_device_chain(rt):
    """D >= max_len: every ended session's fragments are the bytes uvad_fuse -> uvad_cuts_table -> uvad_fuse_pick -> uvad_cuts_gather give
    on the device from the members' whole probabilities and audio."""
    for D in (7, 1000):
        sc, ref, grp, h, b, lo, ms, lag = case(6, np.int16, "lagged", CFG, D, 47, 60)
        got, g = device_run(rt, sc, CFG, D, h, b, lo, ms)
        compare(got, ref, lo, ms)
        n_cuts = 0
        for gi, mine in enumerate(sc["sessions"]):
            rows = sc["groups"][gi]
            for ses in mine:
                n, S = len(ses["labels"]), ses["len"] * 6
                if n == 0:
                    assert device_cuts(got, gi, ses) == []
                    continue
                off = rt.fuse_open([list(range(len(rows)))], mode="max", threshold=0.5)
                fused, glens, labels, best, _ = rt.fuse(torch.from_numpy(ses["probs"]).to(DEV), state=off)
                assert labels[0].cpu().numpy().tobytes() == ses["labels"].tobytes() and best[0].cpu().numpy().tobytes() == ses["best"].tobytes()
                ct = rt.cuts_open(**dict(zip(KEYS, CFG)))
                rt.cuts_table(labels, lengths=glens, S=S, cuts=ct)
                ptab, pick = rt.fuse_pick(best, ct, state=off)
                pcm = torch.from_numpy(np.ascontiguousarray(sc["x"][rows, ses["s0"] * 6:ses["s0"] * 6 + S])).to(DEV)
                batch, blen = rt.cuts_gather(pcm, ct, "samples", table=ptab)
                tab, batch, blen, pick = rt.cuts_read(ct), batch.cpu().numpy(), blen.cpu().numpy(), pick.cpu().numpy()
                cuts = device_cuts(got, gi, ses)
                assert len(cuts) == len(tab)
                for i, (f, k, fl, data, done) in enumerate(cuts):
                    assert (f, k, gg.channel(fl)) == (int(tab[i]["first_frame"]), int(tab[i]["n_frames"]), int(pick[i])) and done
                    assert len(data) == blen[i] == tab[i]["n_samples"] and data.tobytes() == batch[i, :blen[i]].tobytes()
                n_cuts += len(cuts)
        assert n_cuts > 10


def _hand_script(lab, best, chunk=6, way="prompt", dtype=np.int16):
    """One hand-made session on the pair group (rows 0 and 1), the other three groups idle behind junk."""
    n = len(lab)
    n_steps = -(-(n * HOP + TAIL) // 24) * 24 // chunk
    n_all = (n_steps * chunk - TAIL) // HOP
    lab = np.concatenate([np.asarray(lab, np.uint8), np.zeros(n_all - n, np.uint8)])
    best = np.concatenate([np.asarray(best, np.uint8), np.zeros(n_all - n, np.uint8)])
    sessions = [[], [{"s0": 1, "len": n_steps, "labels": lab, "best": best, "way": way}], [], []]
    return make_script(GROUPS, chunk, dtype, n_steps + 2, sessions, tr.LAG0, 3)


def _hand(rt, lab, best, D, pad=0, W=0):
    cfg = (pad, W, 0, HOP, LEAD, TAIL)
    outs = []
    for chunk, way in ((6, "prompt"), (24, "big")):
        sc = _hand_script(lab, best, chunk, way)
        h, b = gg.history(cfg, tr.LAG0, chunk, D), gg.best_history(cfg, tr.LAG0, chunk, D)
        lo, ms = gg.max_out(cfg, sc["ld_lab"], chunk, D), gg.max_seg(cfg, sc["ld_lab"])
        ref, _ = reference(sc, cfg, D, h, b, lo, ms)
        got, _ = device_run(rt, sc, cfg, D, h, b, lo, ms)
        compare(got, ref, lo, ms)
        assert all(int(got[s][2][g]) == 0 for s in range(len(got)) for g in (0, 2, 3))      # the idle groups say nothing
        outs.append([(f, k, gg.channel(fl)) for f, k, fl, d, done in device_cuts(got, 1, sc["sessions"][1][0])])
    assert outs[0] == outs[1]
    return outs[0]


def test_hand_made_cases(rt):
    lab, best = [0, 0] + [1] * 10 + [0] * 4, [0, 0] + [0] * 3 + [1] * 7 + [0] * 4
    assert _hand(rt, lab, best, 3) == [(2, 10, 0)]                          # the first frames' winner is not the cut's
    assert _hand(rt, lab, best, 1000) == [(2, 10, 1)]
    assert _hand(rt, [0] + [1] * 6 + [0] * 3, [0, 1, 0, 1, 0, 1, 0, 0, 0, 0], 6) == [(1, 6, 0)]           # a tie: the lowest position
    assert _hand(rt, [0] + [1] * 6 + [0] * 3, [0, 7, 9, 7, 1, 200, 255, 0, 0, 0], 6) == [(1, 6, 1)]       # bytes past the group's size do not vote
    assert _hand(rt, [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0], 5) == [(3, 2, 1)]   # closes below the horizon
    assert _hand(rt, [0] + [1] * 8 + [0] * 3, [0] + [0] * 4 + [1] * 4 + [0] * 3, 4, W=4) == [(1, 4, 0), (5, 4, 1)]   # split pieces choose apart
    assert _hand(rt, [0] + [1] * 8 + [0] * 5, [1] * 14, 4, pad=1, W=5) == [(0, 5, 1), (5, 5, 1)]           # the interval ends on a piece boundary


def test_overflow_of_max_seg_and_ld_out(rt):
    for ld_out, max_seg in ((40, None), (None, 1), (7, 2), (0, 3), (25, 0)):
        sc, ref, grp, h, b, lo, ms, lag = case(400, np.int16, "one", CFG, 3, 53, 6, ld_out=ld_out, max_seg=max_seg)   # many records a step
        got, g = device_run(rt, sc, CFG, 3, h, b, lo, ms)
        compare(got, ref, lo, ms)
        cut = sum(int((seg["n_stored"] < seg["n"]).sum()) for row in ref for _, seg, _ in row)
        dropped = sum(count - len(seg) for row in ref for _, seg, count in row)
        assert (ld_out is None or cut > 0 or max_seg == 0) and (max_seg is None or dropped > 0)


def test_rings_below_the_bound_zeros_and_lost(rt):
    D = 7
    lag = tr.LAG0 + 5
    full, bfull = gg.history(CFG, lag, 6, D), gg.best_history(CFG, lag, 6, D)
    seen = 0
    for hist, bh in ((full - 5 * HOP, bfull), (full, bfull - 6), (6, 1)):
        sc, ref, grp, h, b, lo, ms, _ = case(6, np.int16, "lagged", CFG, D, 61, 70, hist=hist, bh=bh)
        got, g = device_run(rt, sc, CFG, D, h, b, lo, ms)
        n_rec, n_units, flags = compare(got, ref, lo, ms)
        if hist < full:
            assert flags & gg.LOST
            seen += 1
        else:
            assert not flags & gg.LOST and sum(p.voteless for p in grp) > 0
    assert seen == 2


def test_unsync_and_junk_everywhere_an_idle_group_could_be_read(rt):
    steps = 60
    rflags = np.zeros((steps, B), np.uint8)
    rflags[20, 1] = 1                                                       # row 1 alone says START in step 20: its groups leave lockstep
    rflags[40] = 2                                                          # every row the same: no group minds
    sc, ref, grp, h, b, lo, ms, lag = case(6, np.float32, "prompt", CFG, 3, 71, steps, rflags=rflags)
    got, g = device_run(rt, sc, CFG, 3, h, b, lo, ms)
    n_rec, n_units, flags = compare(got, ref, lo, ms)
    assert flags & gg.UNSYNC
    for s, (out, seg, counts) in enumerate(got):
        for gi in range(4):
            for r in seg[gi, :counts[gi]]:
                assert not (r["flags"] & gg.UNSYNC) or (s >= 20 and gi != 0)        # the one-member group cannot leave lockstep
    assert not np.isnan(np.concatenate([got[s][0][gi, :int(got[s][1][gi, :got[s][2][gi]]["n_stored"].sum())] for s in range(steps)
                                        for gi in range(4)]).view(np.float32)).any()   # row 7's NaN went nowhere
    got2, _ = device_run(rt, sc, CFG, 3, h, b, lo, ms, rflags=False)         # without the rows' bytes: no check
    assert all(not (r["flags"] & gg.UNSYNC) for out, seg, counts in got2 for gi in range(4) for r in seg[gi, :counts[gi]])


def test_same_calls_same_bytes_and_one_graph_for_every_later_step(rt):
    sc, ref, grp, h, b, lo, ms, lag = case(6, np.int16, "bursts", CFG, 3, 83, 70)
    eager, _ = device_run(rt, sc, CFG, 3, h, b, lo, ms)
    again, _ = device_run(rt, sc, CFG, 3, h, b, lo, ms)
    graph, _ = device_run(rt, sc, CFG, 3, h, b, lo, ms, graph_at=4)
    compare(eager, ref, lo, ms)
    for a, other in ((eager, again), (eager, graph)):
        for (o1, s1, c1), (o2, s2, c2) in zip(a, other):
            assert o1.tobytes() == o2.tobytes() and s1.tobytes() == s2.tobytes() and c1.tobytes() == c2.tobytes()


def test_a_group_of_255_members(rt):
    groups = [[(3 * i + 1) % 8 for i in range(255)]]
    sc, ref, grp, h, b, lo, ms, lag = case(6, np.int16, "prompt", (1, 9, 0, HOP, LEAD, TAIL), 5, 97, 40, groups=groups)
    got, g = device_run(rt, sc, (1, 9, 0, HOP, LEAD, TAIL), 5, h, b, lo, ms)
    n_rec, n_units, flags = compare(got, ref, lo, ms)
    chans = {gg.channel(r["flags"]) for out, seg, counts in got for r in seg[0, :counts[0]]}
    print(f"255 members: {n_rec} records, channels {sorted(chans)}")
    assert n_rec > 5 and max(chans) >= 64                                   # a pick past the first wave's positions


def test_collect_and_device_refusals(rt):
    sc, ref, grp, h, b, lo, ms, lag = case(6, np.int16, "prompt", CFG, 3, 31, 90)
    fz = rt.fuse_open(sc["groups"])
    g = rt.gate_group_open(fz, 6, sc["ld_lab"], torch.int16, lag, 3, **dict(zip(KEYS, CFG)))
    assert (g["history"], g["best_history"], g["ld_out"], g["max_seg"]) == (h, b, lo, ms)
    dev = {k: torch.from_numpy(sc[k]).to(DEV) for k in ("labels", "best", "lab_counts", "best_counts", "gflags")}
    x = torch.from_numpy(sc["x"]).to(DEV)
    seen = 0
    for s in range(30):
        fl = dev["gflags"][s]
        rt.gate_group_step(g, x[:, s * 6:(s + 1) * 6].contiguous(), dev["best"][s], dev["best_counts"][s], dev["labels"][s], dev["lab_counts"][s],
                           start=(fl & 1).bool(), end=(fl & 2).bool())
        for gi, recs in enumerate(rt.gate_group_collect(g)):
            want_out, want_seg, want_count = ref[s][gi]
            assert len(recs) == len(want_seg)
            off = 0
            for d, w in zip(recs, want_seg):
                assert (d["index"], d["first_frame"], d["n_frames"], d["offset"], d["n"]) == tuple(int(w[k]) for k in ("index", "first_frame", "n_frames", "offset", "n"))
                assert d["flags"] == int(w["flags"]) & 0xff and d["channel"] == gg.channel(w["flags"]) and d["row"] == sc["groups"][gi][d["channel"]]
                assert d["fragment"].cpu().numpy().tobytes() == want_out[off:off + int(w["n_stored"])].tobytes()
                off += int(w["n_stored"])
                seen += 1
    assert seen > 10
    lib, ctx = rt.lib, rt.ctx
    err = lambda: lib.uvad_last_error(ctx).decode()
    q, st, n = C.byref(g["cfg"]), g["state"].data_ptr(), g["state"].numel()
    big = torch.zeros((B, h + 1), dtype=torch.int16, device=DEV)
    p = lambda k: dev[k][0].data_ptr()
    step = lambda state=st, nbytes=n, chunk=6, rows=B: lib.uvad_gate_group_step(
        ctx, big.data_ptr(), chunk, rows, p("best"), sc["ld_best"], p("best_counts"), p("labels"), sc["ld_lab"], p("lab_counts"), None, None,
        state, nbytes, g["out"].data_ptr(), lo, g["seg"].data_ptr(), ms, g["seg_counts"].data_ptr(), None)
    assert step(chunk=h + 1) == E_ARG and "below chunk" in err()
    assert step(nbytes=n - 1) == E_ARG and f"need {n} bytes" in err()
    assert step(rows=6) == E_ARG and "largest configured member index (6)" in err()
    # big enough, never reset.  The context keeps the states earlier tests reset by address, and the allocator can hand a freed one's block
    # out again: 256 bytes into a block is an address no state of this module ever had (each was the base of its own allocation)
    other = torch.zeros(n + 256, dtype=torch.uint8, device=DEV)[256:]
    assert step(state=other.data_ptr()) == E_STATE and "uvad_gate_group_reset" in err()
    assert lib.uvad_gate_group_reset(ctx, st, n, q, 2, h, b, 0, None) == E_ARG and "decide_frames" in err()
    assert lib.uvad_gate_group_reset(ctx, st, n - 1, q, 2, h, b, 3, None) == E_ARG and f"need {n} bytes" in err()
    rt.fuse_open([[0, 1], [2, 3]])                                          # another configuration in the context: G = 2, N = 4
    assert step() == E_STATE and "G = 4, N = 76" in err()
    with pytest.raises(ValueError, match="bad group gate configuration"):
        rt.gate_group_open(fz, 6, 8, torch.int16, 2, 3, history=5, **dict(zip(KEYS, CFG)))
    with pytest.raises(ValueError, match="bad group gate configuration"):
        rt.gate_group_open(fz, 6, 8, torch.int16, 2, 0, **dict(zip(KEYS, CFG)))
    torch.cuda.synchronize()


def _mono_script(rng, rows, chunk, dtype, steps, hop, tail, hold):
    """Step inputs both gates take: per row, sessions that start and end on the row's own draws; a frame's label arrives once its samples
    and the tail have, up to `hold` frames later, and the END step hands over the rest.  Idle rows and columns past a count hold junk."""
    ld_lab = chunk // hop + hold + 2
    x = rng.integers(-30000, 30000, (steps, rows, chunk)).astype(dtype) if np.dtype(dtype).kind == "i" else \
        rng.uniform(-1.0, 1.0, (steps, rows, chunk)).astype(dtype)
    labels = rng.integers(0, 256, (steps, rows, ld_lab)).astype(np.uint8)
    counts = rng.integers(-3, ld_lab + 4, (steps, rows)).astype(np.int32)
    flags = np.zeros((steps, rows), np.uint8)
    for b in range(rows):
        s = int(rng.integers(0, 3))
        while s < steps:
            n_steps = min(int(rng.integers(1, 14)), steps - s)
            lab, d = tg.random_labels(rng, n_steps * chunk // hop + 1), 0
            for i in range(n_steps):
                last = i == n_steps - 1
                avail = max(((i + 1) * chunk - tail) // hop, 0)
                d1 = avail if last else max(d, avail - int(rng.integers(0, hold + 1)))
                assert d1 - d <= ld_lab
                labels[s + i, b, :d1 - d], counts[s + i, b] = lab[d:d1], d1 - d
                flags[s + i, b] = (gg.START if i == 0 else 0) | (gg.END if last else 0)
                d = d1
            s += n_steps + int(rng.integers(0, 3))
    return x, labels, counts, flags, ld_lab


def _both_gates(rt, cfg, x, labels, counts, flags, ld_lab, lag, hist, ld_out, max_seg):
    """The same steps through the mono gate (one slot per row) and the group gate (one one-member group per row, decide_frames = 1, no row
    flags) -> per step the two (out, seg, seg_counts), every buffer pre-filled with the canary."""
    steps, rows, chunk = x.shape
    dt, kw = TORCH[x.dtype], dict(zip(KEYS, cfg))
    mono = rt.gate_open(rows, chunk, ld_lab, dt, lag, history=hist, ld_out=ld_out, max_seg=max_seg, **kw)
    grp = rt.gate_group_open(rt.fuse_open([[r] for r in range(rows)]), chunk, ld_lab, dt, lag, 1, history=hist, ld_out=ld_out, max_seg=max_seg, **kw)
    assert mono["history"] == grp["history"] and mono["out"].shape == grp["out"].shape and mono["seg"].shape == grp["seg"].shape
    dx, dl, dc, df = (torch.from_numpy(v).to(DEV) for v in (x, labels, counts, flags))
    best = torch.zeros((rows, ld_lab), dtype=torch.uint8, device=DEV)       # one member: position 0 wins every frame
    got = []
    for s in range(steps):
        for g in (mono, grp):
            g["out"].view(torch.uint8).fill_(CANARY)
            g["seg"].view(torch.uint8).fill_(CANARY)
            g["seg_counts"].fill_(-7)
        start, end = (df[s] & 1).bool(), (df[s] & 2).bool()
        rt.gate_step(mono, dx[s], dl[s], dc[s], start=start, end=end)
        rt.gate_group_step(grp, dx[s], best, dc[s], dl[s], dc[s], start=start, end=end)
        got.append([v.clone() for g in (mono, grp) for v in (g["out"], g["seg"], g["seg_counts"])])
    torch.cuda.synchronize()
    return [[v.cpu().numpy() for v in row] for row in got], mono


def test_one_member_groups_at_decide_1_are_the_mono_gate(rt):
    """With one member and decide_frames = 1 nothing is deferred and the channel bits are 0: step by step the group gate's counts, records
    and output bytes are the mono gate's on the same rows (the two slot layouts differ: outputs only).  The two restatements agree byte
    for byte under this setting; the mono one runs here for its trace, so that the comparison cannot pass on empty sessions."""
    hop, lead, tail, hold, rows, steps = 2, 1, 3, 3, 4, 40
    lag = hold + -(-tail // hop)
    runs = [(chunk, dtype, pad, W, 1, None, None) for chunk in (6, 10) for dtype in (np.int16, np.float32) for pad in (0, 2) for W in (0, 3)]
    runs += [(6, np.int16, 2, 3, 2, None, None), (10, np.float32, 2, 3, 1, 3, 2)]       # the history halved; ld_out cut to a third, max_seg = 2
    runs += [(10, np.int16, 2, 0, 1, 8, None)]                                          # long pieces into an eighth of ld_out: fragments are cut
    trace, n_rec, lost, cut, dropped = set(), 0, 0, 0, 0
    for i, (chunk, dtype, pad, W, shrink, out_div, max_seg) in enumerate(runs):
        cfg = (pad, W, 0, hop, lead, tail)
        x, labels, counts, flags, ld_lab = _mono_script(np.random.default_rng(500 + i), rows, chunk, dtype, steps, hop, tail, hold)
        hist = max(gr.history(cfg, lag, chunk) // shrink, chunk)
        assert gg.history(cfg, lag, chunk, 1) == gr.history(cfg, lag, chunk)
        ld_out = gr.max_out(cfg, ld_lab, chunk) // (out_div or 1)
        ms = gr.max_seg(cfg, ld_lab) if max_seg is None else max_seg
        got, mono = _both_gates(rt, cfg, x, labels, counts, flags, ld_lab, lag, hist, ld_out, ms)
        ref, slots = gr.simulate(cfg, hist, x, labels, counts, flags, ld_out, ms)
        trace |= set().union(*(sl.trace for sl in slots))
        for s, (o1, s1, c1, o2, s2, c2) in enumerate(got):
            assert c1.tolist() == c2.tolist() == [count for _, _, count in ref[s]], (i, s)
            assert s1.tobytes() == s2.tobytes(), (i, s)
            assert o1.tobytes() == o2.tobytes(), (i, s)
            seg = s1.view(gr.SEG_DTYPE).reshape(rows, -1)
            for b in range(rows):
                k = min(int(c1[b]), ms)
                n_rec += k
                lost += int((seg[b, :k]["flags"] & gr.LOST != 0).sum())
                cut += int((seg[b, :k]["n_stored"] < seg[b, :k]["n"]).sum())
                dropped += int(c1[b]) - k
                assert not (seg[b, :k]["flags"] >> 4).any()                 # neither UNSYNC nor a channel
    print(f"{len(runs)} configurations: {n_rec} records, {lost} LOST, {cut} truncated, {dropped} dropped, met {sorted(trace)}")
    assert {"split", "rejoin", "ring wrap"} <= trace and n_rec > 400 and lost > 0 and cut > 0 and dropped > 0
