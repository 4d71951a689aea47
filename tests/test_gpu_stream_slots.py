"""GPU tests (-m gpu) of the causal stream's slot pool (uvad_stream_slots_*, VadRuntime.stream_slots_*): B slots in lockstep, each holding
at most one session that starts and ends on its own flag bits, the whole step one launch of lstm_stack_slots_kernel.

  identity   every session is, bit for bit and step for step, the B = 1 uvad_stream_step stream reset at its start and fed the same
             chunks; the tile mixes k_b of 0 .. 4 (chunks 160 .. 640, staggered starts), odd and even frame pairings included
  offline    the same sessions against uvad_forward on each session's whole audio within test_gpu_stream_paths.LOGIT_TOL
  canary     outputs [B + 1][kmax + 3] and counts [B + 1] pre-filled: only n_b columns of row b and B counts change; idle slots' chunk
             rows hold NaN / Inf throughout; one non-finite sample poisons its own session only, until the slot's next START
  one graph  the first step is captured, every later step of the churn schedule replayed, also with the GPU idle between replays
  the chain  endpointers, gate, fusion and group gate behind the pool equal the same stages run by hand on the pool's recorded outputs
  plus the refusals and the named size (512 slots x 320 samples under churn).

Models and sizes are those of test_gpu_stream_paths.py's A-* cases (weights x 2; 64 povey / 80 hamming features; 1 / 4 layers; 0 / 2
feed-forward layers); B = 7 slots is two tiles, the second with a padding sequence; sessions last 1 - 1.5 s.

Probabilities: uvad_stream_step has no probability output, so the pool's probabilities are held to the float64 sigmoid of the
(bit-identical) logits within PROB_TOL = 4 * 2^-24: expf (<= 1 ulp), one addition and one correctly rounded division on a value
below 1 stay below 3 ulp of 1 = 3 * 2^-24; and to bit equality wherever two pool runs are compared."""
import functools

import numpy as np
import pytest
import torch

import stream_ref as sr
import test_gpu_stream_paths as sp

pytestmark = pytest.mark.gpu

DEV = sp.DEV
B7 = sp.B7
LOGIT_TOL = sp.LOGIT_TOL
PROB_TOL = 4 * 2.0 ** -24
E_ARG, E_STATE, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4, -5      # include/uvad.h
CHUNKS = (160, 250, 320, 480, 560, 640)
CANARY = -7.25
MODELS = {
    "f64-l1-ff2": sp.cfg("A", 320, layers=1),
    "f64-l4-ff0": sp.cfg("A", 320, lin=(128, 0)),
    "f80-l1-ff0": sp.cfg("A", 320, F=80, window="hamming", layers=1, lin=(128, 0)),
    "f80-l4-ff2": sp.cfg("A", 320, F=80, window="hamming"),
}


def kmax_of(chunk):
    return -(-chunk // 160)


def schedule(chunk, B=B7):
    """Flags (steps, B) with sessions of 1 - 1.5 s (n1 steps = 1 s).  Tile 0: slots 0 .. 3 start at steps 0, 1, 2, 3; slot 0 ENDs and
    STARTs again in the next step; slot 1 is STARTed again while active; slot 2 begins with a one-chunk session (START | END).  Tile 1
    is all idle for the first second; slot 6 is idle for 1.5 s before its first START and sees an END while idle; slot 4 never ends."""
    n1 = 16000 // chunk
    steps = 2 * n1 + n1 // 2 + 8
    f = np.zeros((steps, B), np.uint8)
    f[0, 0], f[n1 + 2, 0], f[n1 + 3, 0] = 1, 2, 1
    f[1, 1], f[1 + n1 // 3, 1], f[1 + n1 // 3 + n1, 1] = 1, 1, 2
    f[2, 2], f[4, 2], f[4 + n1 + n1 // 2 - 1, 2] = 3, 1, 2
    f[3, 3], f[3 + n1, 3] = 1, 2
    f[n1, 4] = 1
    f[n1 + 2, 5], f[2 * n1 + 2, 5] = 1, 2
    f[5, 6], f[n1 + n1 // 2, 6] = 2, 1
    return f


def sessions(flags):
    """[(slot, first step, last step)] of a schedule."""
    steps, B = flags.shape
    out = []
    for b in range(B):
        s0 = None
        for s in range(steps):
            if flags[s, b] & 1:
                if s0 is not None:
                    out.append((b, s0, s - 1))
                s0 = s
            if flags[s, b] & 2 and s0 is not None:
                out.append((b, s0, s))
                s0 = None
        if s0 is not None:
            out.append((b, s0, steps - 1))
    return out


def live_mask(flags):
    """(steps, B) bool: the slot holds a session in that step."""
    live = np.zeros(flags.shape, bool)
    cur = np.zeros(flags.shape[1], bool)
    for s in range(flags.shape[0]):
        cur = cur | (flags[s] & 1 == 1)
        live[s] = cur
        cur = cur & ~(flags[s] & 2 == 2)
    return live


@functools.lru_cache(maxsize=None)
def pcm(B, S, seed=4200):
    from uvad_amd.synth import synth_pcm
    return torch.from_numpy(synth_pcm(B, S, seed=seed)).to(DEV)


def chunks_of(x, flags, chunk, poison=True):
    """The (B, chunk) block of every step; the rows of idle slots hold NaN (even steps) or Inf (odd steps)."""
    live = live_mask(flags)
    out = []
    for s in range(flags.shape[0]):
        xs = x[:flags.shape[1], s * chunk:(s + 1) * chunk].clone()
        if poison:
            xs[torch.from_numpy(~live[s]).to(DEV)] = float("nan") if s % 2 == 0 else float("inf")
        out.append(xs)
    return out


def run_raw(rt, blocks, flags, chunk):
    """The C entry itself, step by step, on canary-filled outputs one row and three columns larger than it may touch.
    -> per step (logits (B, kmax), probs (B, kmax), counts (B,)) host arrays; the canary is checked in every step."""
    lib, ctx = rt.lib, rt.ctx
    steps, B = flags.shape
    kmax = kmax_of(chunk)
    assert lib.uvad_stream_slots_kmax(ctx, chunk) == kmax
    state = torch.empty(int(lib.uvad_stream_slots_state_bytes(ctx, B)), dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(lib.uvad_stream_slots_workspace_bytes(ctx, B, chunk)), dtype=torch.uint8, device=DEV)
    rt._check(lib.uvad_stream_slots_reset(ctx, state.data_ptr(), B, chunk, rt._stream()))
    ld = kmax + 3
    dflags = torch.from_numpy(flags).to(DEV)
    out = []
    for s in range(steps):
        lg = torch.full((B + 1, ld), CANARY, device=DEV)
        pr = torch.full((B + 1, ld), CANARY, device=DEV)
        cnt = torch.full((B + 1,), -77, dtype=torch.int32, device=DEV)
        rt._check(lib.uvad_stream_slots_step(ctx, blocks[s].data_ptr(), dflags[s].data_ptr(), B, chunk, state.data_ptr(), lg.data_ptr(),
                                             pr.data_ptr(), ld, cnt.data_ptr(), ws.data_ptr(), ws.numel(), rt._stream()))
        lg, pr, cnt = lg.cpu().numpy(), pr.cpu().numpy(), cnt.cpu().numpy()
        assert cnt[B] == -77 and (lg[B] == CANARY).all() and (pr[B] == CANARY).all(), s
        for b in range(B):
            n = int(cnt[b])
            assert 0 <= n <= kmax, (s, b, n)
            assert (lg[b, n:] == CANARY).all() and (pr[b, n:] == CANARY).all(), (s, b, n)
        out.append((lg[:B, :kmax].copy(), pr[:B, :kmax].copy(), cnt[:B].copy()))
    return out


_BASE = {}


def base(model, chunk):
    """The shared run of a (model, chunk): (rt, x, flags, blocks, per-step outputs, per-session B = 1 references).  Computed once."""
    key = (model, chunk)
    if key not in _BASE:
        c = MODELS[model]
        rt = sp.runtime(c)
        flags = schedule(chunk)
        x = pcm(B7, flags.shape[0] * chunk)
        blocks = chunks_of(x, flags, chunk)
        got = run_raw(rt, blocks, flags, chunk)
        refs = {}
        for b, s0, s1 in sessions(flags):
            st = rt.stream_open(1, chunk)
            refs[(b, s0, s1)] = [rt.stream_step(st, x[b:b + 1, s * chunk:(s + 1) * chunk].contiguous()).cpu().numpy()[0].copy()
                                 for s in range(s0, s1 + 1)]
        _BASE[key] = (rt, x, flags, blocks, got, refs)
    return _BASE[key]


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("model", list(MODELS))
def test_every_session_is_its_single_feed_stream_bit_for_bit(model, chunk):
    from uvad_amd.runtime import stream_slots_plan
    rt, x, flags, blocks, got, refs = base(model, chunk)
    steps = flags.shape[0]
    plan = stream_slots_plan(flags, chunk)
    live = live_mask(flags)
    for s in range(steps):
        want = [hi - lo for (_, lo, hi, _) in plan[s]]
        assert got[s][2].tolist() == want, (s, got[s][2].tolist(), want)
        assert all(got[s][2][b] == 0 for b in range(B7) if not live[s, b])
    mixes, seen_k = set(), set()
    for s in range(steps):
        for tile in (slice(0, 4), slice(4, B7)):
            ks = tuple(int(k) for k, on in zip(got[s][2][tile], live[s][tile]) if on)
            if len(set(ks)) > 1:
                mixes.add(tuple(sorted(set(ks))))
            seen_k |= set(ks)
    assert mixes, "no tile ever mixed two frame counts"
    assert kmax_of(chunk) in seen_k and len(seen_k) > 1, seen_k
    frames = 0
    for (b, s0, s1), ref in refs.items():
        for s in range(s0, s1 + 1):
            n = int(got[s][2][b])
            want = ref[s - s0]
            assert n == len(want), (b, s0, s, n, len(want))
            assert got[s][0][b, :n].tobytes() == want.tobytes(), (b, s0, s, got[s][0][b, :n], want)
            p64 = 1.0 / (1.0 + np.exp(-want.astype(np.float64)))
            assert n == 0 or np.abs(got[s][1][b, :n].astype(np.float64) - p64).max() <= PROB_TOL, (b, s0, s)
            frames += n
        assert sum(len(r) for r in ref) == sr.frames_complete((s1 + 1 - s0) * chunk)
    print(f"stream slots {model} chunk {chunk}: {len(refs)} sessions, {frames} frames bitwise, k mixes inside a tile {sorted(mixes)}")
    assert frames > 0 and np.isfinite(np.concatenate([np.concatenate(r) for r in refs.values()])).all()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("model", list(MODELS))
def test_every_session_equals_the_offline_path(model, chunk):
    rt, x, flags, blocks, got, refs = base(model, chunk)
    worst = 0.0
    for (b, s0, s1) in refs:
        mine = np.concatenate([got[s][0][b, :int(got[s][2][b])] for s in range(s0, s1 + 1)])
        if len(mine) == 0:
            continue
        offline, _ = rt.forward(x[b:b + 1, s0 * chunk:(s1 + 1) * chunk].contiguous())
        offline = offline.cpu().numpy()[0]
        assert len(mine) <= len(offline)
        worst = max(worst, float(np.abs(mine - offline[:len(mine)]).max()))
    print(f"stream slots {model} chunk {chunk}: |pool - offline| {worst:.2e}")
    assert worst < LOGIT_TOL


def test_a_non_finite_sample_poisons_its_own_session_only():
    """One NaN sample in slot 1's chunk while its session runs: no bit of any other slot changes in any step, slot 1 turns non-finite,
    and after slot 1's next START its frames are again those of a fresh session."""
    model, chunk = "f64-l4-ff0", 320
    rt, x, flags, blocks, got, refs = base(model, chunk)
    restart = 1 + (16000 // chunk) // 3
    assert flags[1, 1] == 1 and flags[restart, 1] == 1 and restart > 6
    dirty = [b.clone() for b in blocks]
    dirty[4][1, 17] = float("nan")
    bad = run_raw(rt, dirty, flags, chunk)
    hit = False
    for s in range(flags.shape[0]):
        assert (bad[s][2] == got[s][2]).all(), s
        for b in range(B7):
            n = int(got[s][2][b])
            if b == 1 and 4 <= s < restart:
                hit |= n > 0 and not np.isfinite(bad[s][0][b, :n]).all()
                continue
            assert bad[s][0][b, :n].tobytes() == got[s][0][b, :n].tobytes(), (s, b)
            assert bad[s][1][b, :n].tobytes() == got[s][1][b, :n].tobytes(), (s, b)
    assert hit, "the NaN sample never reached slot 1's logits: the test has no teeth"


def run_pool(rt, blocks, flags, chunk, graphs=False, sync=False, **chain):
    """Every step through VadRuntime.stream_slots_step -> (per step dicts of host arrays, the pool)."""
    steps, B = flags.shape
    st = rt.stream_slots_open(B, chunk, graphs=graphs, **chain)
    out = []
    for s in range(steps):
        if sync:
            torch.cuda.synchronize()
        fl = flags[s]
        lg, cnt = rt.stream_slots_step(st, blocks[s], start=fl & 1 == 1, end=fl & 2 == 2) if fl.any() else rt.stream_slots_step(st, blocks[s])
        rec = {"logits": lg.clone(), "counts": cnt.clone()}
        if "probs" in st:
            rec["probs"] = st["probs"].clone()
        for stage, keys in (("endpoint", ("events", "ev_counts", "active", "labels", "lab_counts")), ("gate", ("out", "seg", "seg_counts")),
                            ("fuse", ("fused", "glens", "best", "flags")), ("group_gate", ("out", "seg", "seg_counts"))):
            if st.get(stage) is not None:
                rec.update({f"{stage}.{k}": st[stage][k].clone() for k in keys})
        out.append(rec)
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in rec.items()} for rec in out], st


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("model,chunk", [("f64-l4-ff0", 250), ("f80-l4-ff2", 560)])
def test_one_captured_graph_replays_the_whole_schedule(model, chunk, sync):
    """sync: a device synchronise before every step, so each replay starts on an idle GPU."""
    rt, x, flags, blocks, got, refs = base(model, chunk)
    replay, st = run_pool(rt, blocks, flags, chunk, graphs=True, sync=sync)
    assert st["graphs"] == 1 and st["out"].shape == (B7, kmax_of(chunk))
    for s in range(flags.shape[0]):
        assert (replay[s]["counts"] == got[s][2]).all(), s
        for b in range(B7):
            n = int(got[s][2][b])
            assert replay[s]["logits"][b, :n].tobytes() == got[s][0][b, :n].tobytes(), (s, b)


def _thresholds(got):
    emitted = np.concatenate([g[1][b, :int(g[2][b])] for g in got for b in range(g[2].shape[0])]).astype(np.float64)
    assert len(emitted) > 50
    return [float(np.float32(np.percentile(emitted, p))) for p in (40, 50, 60)]


def _same_rows(a, b, n, what):
    assert a.shape[0] == b.shape[0] == len(n), what
    for i, k in enumerate(n):
        assert a[i, :int(k)].tobytes() == b[i, :int(k)].tobytes(), (what, i)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("kind", ["hyst", "hyst-spread", "median"])
def test_endpointer_and_gate_behind_the_pool_equal_the_stages_by_hand(kind, graphs):
    """hyst: onset 0.6 / offset 0.4 as they stand; hyst-spread and median: thresholds at percentiles of the probabilities this model
    emits, so that labels fall on both sides and events, labels and gate records are certain to exist."""
    model, chunk = "f64-l1-ff2", 320
    rt, x, flags, blocks, got, refs = base(model, chunk)
    clean = chunks_of(x, flags, chunk, poison=False)      # the gate copies samples: finite rows, so that bytes compare
    lo, mid, hi = _thresholds(got)
    ep_cfg = {"hyst": {"onset": 0.6, "offset": 0.4, "min_on": 3, "min_off": 2}, "hyst-spread": {"onset": hi, "offset": lo, "min_on": 3, "min_off": 2},
              "median": {"kernel": 5, "pad": 1, "threshold": mid}}[kind]
    kind, spread = kind.split("-")[0], kind != "hyst"
    run, st = run_pool(rt, clean, flags, chunk, graphs=graphs, endpoint=ep_cfg, gate={"max_len": 40})
    if graphs:
        assert st["graphs"] == 1
    ep0, g0 = st["endpoint"], st["gate"]
    ld = kmax_of(chunk)
    ep = rt.endpoint_hyst_open(B7, ld, **ep_cfg) if kind == "hyst" else rt.endpoint_open(B7, ld, **ep_cfg)
    step = rt.endpoint_hyst_step if kind == "hyst" else rt.endpoint_step
    gate = rt.gate_open(B7, chunk, ep["labels"].shape[1], torch.float32, g0["lag_frames"], max_len=40, hop=160, lead=120, tail=120)
    assert gate["history"] == g0["history"] and gate["ld_out"] == g0["ld_out"] and gate["max_seg"] == g0["max_seg"]
    n_events = n_labels = n_seg = 0
    for s in range(flags.shape[0]):
        r, fl = run[s], flags[s]
        # the pool's outputs are not moved by the nodes behind it
        assert (r["counts"] == got[s][2]).all()
        _same_rows(r["logits"], got[s][0], got[s][2], ("logits", s))
        _same_rows(r["probs"], got[s][1], got[s][2], ("probs", s))
        probs = torch.from_numpy(np.ascontiguousarray(r["probs"])).to(DEV)
        counts = torch.from_numpy(r["counts"]).to(DEV)
        kw = dict(start=fl & 1 == 1, end=fl & 2 == 2) if fl.any() else {}
        ev, evc, act = step(ep, probs, counts, **kw)
        out, seg, segc = rt.gate_step(gate, clean[s], ep["labels"], ep["lab_counts"], **kw)
        evc, labc, segc = evc.cpu().numpy(), ep["lab_counts"].cpu().numpy(), segc.cpu().numpy()
        assert (r["endpoint.ev_counts"] == evc).all() and (r["endpoint.lab_counts"] == labc).all(), s
        assert (r["endpoint.active"] == act.cpu().numpy()).all() and (r["gate.seg_counts"] == segc).all(), s
        ev, seg, out, lab = ev.cpu().numpy(), seg.cpu().numpy(), out.cpu().numpy(), ep["labels"].cpu().numpy()
        for b in range(B7):
            ne, nl, ns = min(int(evc[b]), ev.shape[1]), int(labc[b]), min(int(segc[b]), seg.shape[1])
            assert r["endpoint.events"][b, :ne].tobytes() == ev[b, :ne].tobytes(), (s, b)
            assert r["endpoint.labels"][b, :nl].tobytes() == lab[b, :nl].tobytes(), (s, b)
            assert r["gate.seg"][b, :ns].tobytes() == seg[b, :ns].tobytes(), (s, b)
            used = int(seg[b, :ns, 7].sum())
            assert r["gate.out"][b, :used].tobytes() == out[b, :used].tobytes(), (s, b)
            n_events, n_labels, n_seg = n_events + ne, n_labels + nl, n_seg + ns
    print(f"chain {kind} graphs={graphs}: {n_events} events, {n_labels} labels, {n_seg} gate records")
    assert not spread or (n_events > 0 and n_labels > 0 and n_seg > 0)


@pytest.mark.parametrize("graphs", [False, True])
def test_fusion_and_group_gate_behind_the_pool_equal_the_stages_by_hand(graphs):
    """3 two-channel groups; the members of a group share their flags (lockstep), the groups start and end on their own."""
    model, chunk, B, groups = "f64-l1-ff2", 320, 6, [[0, 1], [2, 3], [4, 5]]
    rt = sp.runtime(MODELS[model])
    gflags = schedule(chunk, B=7)[:, [0, 2, 5]]
    flags = np.repeat(gflags, 2, axis=1)
    x = pcm(B7, flags.shape[0] * chunk)
    clean = chunks_of(x, flags, chunk, poison=False)
    bare, _ = run_pool(rt, clean, flags, chunk)
    bare_p, _ = run_pool(rt, clean, flags, chunk, endpoint={"onset": 0.5})
    emitted = np.concatenate([r["probs"][b, :int(r["counts"][b])] for r in bare_p for b in range(B)]).astype(np.float64)
    EP = {"onset": float(np.float32(np.percentile(emitted, 60))), "offset": float(np.float32(np.percentile(emitted, 40))), "min_on": 3, "min_off": 2}
    FZ = {"groups": groups, "mode": "max", "threshold": EP["onset"]}
    GATE = {"decide_frames": 5, "max_len": 40}
    run, st = run_pool(rt, clean, flags, chunk, graphs=graphs, fuse=FZ, endpoint=EP, group_gate=GATE)
    if graphs:
        assert st["graphs"] == 1
    gg0 = st["group_gate"]
    ld = kmax_of(chunk)
    fz = rt.fuse_open(groups, mode="max", threshold=EP["onset"])
    ep = rt.endpoint_hyst_open(3, ld, **EP)
    gg = rt.gate_group_open(fz, chunk, ep["labels"].shape[1], torch.float32, gg0["lag_frames"], 5, max_len=40, hop=160, lead=120, tail=120)
    assert (gg["history"], gg["best_history"], gg["ld_out"], gg["max_seg"]) == (gg0["history"], gg0["best_history"], gg0["ld_out"], gg0["max_seg"])
    n_seg = n_events = 0
    for s in range(flags.shape[0]):
        r, fl, gf = run[s], flags[s], gflags[s]
        assert (r["counts"] == bare[s]["counts"]).all()
        _same_rows(r["logits"], bare[s]["logits"], bare[s]["counts"], ("logits", s))
        _same_rows(r["probs"], bare_p[s]["probs"], bare[s]["counts"], ("probs", s))
        probs = torch.from_numpy(np.ascontiguousarray(r["probs"])).to(DEV)
        counts = torch.from_numpy(r["counts"]).to(DEV)
        fused, glens, _, best, _ = rt.fuse(probs, lengths=counts, state=fz, labels=False, best=True)
        gl = glens.cpu().numpy()
        assert (r["fuse.glens"] == gl).all(), s
        assert (r["fuse.flags"] == gf).all() or not (fl.any() or graphs), s      # (eager steps without flags pass NULL: no OR-ed flags written)
        _same_rows(r["fuse.fused"], fused.cpu().numpy(), gl, ("fused", s))
        _same_rows(r["fuse.best"], best.cpu().numpy(), gl, ("best", s))
        kw = dict(start=gf & 1 == 1, end=gf & 2 == 2) if gf.any() else {}
        ev, evc, act = rt.endpoint_hyst_step(ep, fused, glens, **kw)
        out, seg, segc = rt.gate_group_step(gg, clean[s], best, glens, ep["labels"], ep["lab_counts"],
                                            row_flags=torch.from_numpy(fl.copy()).to(DEV) if fl.any() else None, **kw)
        evc, labc, segc = evc.cpu().numpy(), ep["lab_counts"].cpu().numpy(), segc.cpu().numpy()
        assert (r["endpoint.ev_counts"] == evc).all() and (r["endpoint.lab_counts"] == labc).all(), s
        assert (r["endpoint.active"] == act.cpu().numpy()).all() and (r["group_gate.seg_counts"] == segc).all(), s
        ev, seg, out, lab = ev.cpu().numpy(), seg.cpu().numpy(), out.cpu().numpy(), ep["labels"].cpu().numpy()
        for g in range(3):
            ne, nl, ns = min(int(evc[g]), ev.shape[1]), int(labc[g]), min(int(segc[g]), seg.shape[1])
            assert r["endpoint.events"][g, :ne].tobytes() == ev[g, :ne].tobytes(), (s, g)
            assert r["endpoint.labels"][g, :nl].tobytes() == lab[g, :nl].tobytes(), (s, g)
            assert r["group_gate.seg"][g, :ns].tobytes() == seg[g, :ns].tobytes(), (s, g)
            used = int(seg[g, :ns, 7].sum())
            assert r["group_gate.out"][g, :used].tobytes() == out[g, :used].tobytes(), (s, g)
            n_seg, n_events = n_seg + ns, n_events + ne
    print(f"fused chain graphs={graphs}: {n_events} events, {n_seg} group gate records")
    assert n_events > 0 and n_seg > 0


def _rt(F=64, window="povey", **model):
    import uvad_amd
    from oracle import torch_ref as tr
    q = dict(hidden=128, layers=2, bidirectional=False, lin=(128, 1), snip_edges=False)
    q.update(model)
    cfg = {"encoding_dim": F, "lstm": {"hidden_size": q["hidden"], "num_layers": q["layers"], "bidirectional": q["bidirectional"]},
           "linear": {"hidden_size": q["lin"][0], "num_layers": q["lin"][1]}, "leaky_slope": 0.01}
    rt = uvad_amd.VadRuntime(DEV, fbank=uvad_amd.FbankConfig(num_filters=F, window_type=window, snip_edges=q["snip_edges"]), model=cfg)
    rt.load_state_dict(tr.seeded_state_dict(F, q["hidden"], q["layers"], q["bidirectional"], q["lin"][0], q["lin"][1], seed=1234, scale=2.0))
    return rt


def test_stream_slots_refusals_each_leaving_the_state_usable():
    B, chunk = 5, 320
    kmax = kmax_of(chunk)

    def reset(rt, state, b=B, ch=chunk):
        return rt.lib.uvad_stream_slots_reset(rt.ctx, state.data_ptr(), b, ch, rt._stream())

    # ---- models and framings the one-launch step does not take: refused by reset with a text that names the limit
    for kw, word in ((dict(bidirectional=True), "causal"), (dict(hidden=64), "hidden_size 128"), (dict(layers=9), "layers"),
                     (dict(F=40), "64 or 80 features"), (dict(lin=(64, 1)), "128 -> 128"), (dict(snip_edges=True), "snip_edges")):
        F = kw.pop("F", 64)
        rt = _rt(F=F, **kw)
        state = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
        assert reset(rt, state) == E_UNSUPPORTED, kw
        msg = rt.lib.uvad_last_error(rt.ctx).decode()
        assert word in msg, (kw, msg)
        with pytest.raises(Exception):
            rt.stream_slots_open(B, chunk)
    # ---- a model it takes
    rt = sp.runtime(MODELS["f64-l1-ff2"])
    lib, ctx = rt.lib, rt.ctx
    state = torch.empty(int(lib.uvad_stream_slots_state_bytes(ctx, B)), dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(lib.uvad_stream_slots_workspace_bytes(ctx, B, chunk)), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0
    x = pcm(B7, 16000)[:B, :chunk].contiguous()
    out = torch.full((B, kmax), CANARY, device=DEV)
    prb = torch.full((B, kmax), CANARY, device=DEV)
    cnt = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    flags = torch.ones(B, dtype=torch.uint8, device=DEV)

    def step(b=B, ch=chunk, ld=kmax, wsb=None, st=state, counts=cnt, lg=out, pr=prb):
        return lib.uvad_stream_slots_step(ctx, x.data_ptr(), flags.data_ptr(), b, ch, st.data_ptr(), lg.data_ptr() if lg is not None else None,
                                          pr.data_ptr() if pr is not None else None, ld, counts.data_ptr() if counts is not None else None,
                                          ws.data_ptr(), ws.numel() if wsb is None else wsb, rt._stream())

    assert step() == E_STATE                                     # never reset
    assert reset(rt, state, ch=641) == E_ARG and "ceil" in lib.uvad_last_error(ctx).decode()       # 5 frames in a step
    assert reset(rt, state, ch=119) == E_ARG and "first" in lib.uvad_last_error(ctx).decode()      # chunk < (400 - 160) / 2
    assert step() == E_STATE                                     # a refused reset registers nothing
    assert reset(rt, state) == 0
    assert step(b=B + 1) == E_ARG
    assert step(ch=chunk - 1) == E_ARG
    assert step(ld=kmax - 1) == E_ARG
    assert step(counts=None) == E_ARG
    assert step(lg=None, pr=None) == E_ARG
    assert step(wsb=ws.numel() - 1) == E_WORKSPACE
    other = torch.empty_like(state)
    assert step(st=other) == E_STATE
    torch.cuda.synchronize()
    assert int((cnt != -77).sum()) == 0 and bool((out == CANARY).all()) and bool((prb == CANARY).all())      # nothing was enqueued
    # the state is as the reset left it: the step now runs, every slot starts, and a 320-sample first chunk completes one frame
    assert step() == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [1] * B
    ref = rt.stream_step(rt.stream_open(B, chunk), x)
    assert torch.equal(out[:, :1], ref) and bool((out[:, 1:] == CANARY).all())
    # either output alone
    assert reset(rt, state) == 0 and step(pr=None) == 0 and reset(rt, state) == 0 and step(lg=None) == 0
    torch.cuda.synchronize()
    # uvad_stream_slots_kmax over the chunks 120 .. 700, and its refusals
    for ch in range(120, 701):
        assert lib.uvad_stream_slots_kmax(ctx, ch) == -(-ch // 160), ch
    assert lib.uvad_stream_slots_kmax(ctx, 0) < 0 and lib.uvad_stream_slots_kmax(ctx, -3) < 0
    # a context without a model: the configuration is missing
    from uvad_amd.features import FbankConfig
    from uvad_amd.runtime import VadRuntime
    bare = VadRuntime(DEV, fbank=FbankConfig(num_filters=64))
    assert bare.lib.uvad_stream_slots_state_bytes(bare.ctx, B) == 0
    assert bare.lib.uvad_stream_slots_reset(bare.ctx, state.data_ptr(), B, chunk, bare._stream()) == E_STATE


def test_named_size_512_slots_20ms_60_steps_under_churn():
    """512 slots x 320 samples, 60 steps; every slot starts at one of a few steps, about a quarter are idle at any time, sessions end and
    restart throughout.  Sessions that share a start step are compared with ONE lockstep uvad_stream_step group of that size (feeds of
    the one-launch path are independent bit for bit); 16 sessions with their B = 1 streams; every count with the plan."""
    from uvad_amd.runtime import stream_slots_plan
    B, chunk, steps = 512, 320, 60
    rt = sp.runtime(MODELS["f64-l4-ff0"])
    rng = np.random.default_rng(512)
    flags = np.zeros((steps, B), np.uint8)
    for b in range(B):
        s = int(rng.choice([0, 0, 0, 1, 2, 5, 9]))
        while s < steps:
            n = int(rng.choice([1, 6, 12, 20, 33, 60]))
            flags[s, b] |= 1
            if s + n - 1 < steps:
                flags[s + n - 1, b] |= 2
            s += n + int(rng.choice([0, 4, 8, 10, 16]))
    live = live_mask(flags)
    assert 0.15 < 1.0 - live[10:].mean() < 0.4 and (flags & 1).any(axis=1).sum() >= 50 and (flags & 2).any(axis=1).sum() >= 50      # the schedule churns
    x = pcm(B, steps * chunk, seed=4512)
    blocks = chunks_of(x, flags, chunk)
    st = rt.stream_slots_open(B, chunk, graphs=True)
    outs, counts = [], []
    for s in range(steps):
        fl = flags[s]
        lg, cnt = rt.stream_slots_step(st, blocks[s], start=fl & 1 == 1, end=fl & 2 == 2)
        outs.append(lg.clone())
        counts.append(cnt.clone())
    assert st["graphs"] == 1
    outs, counts = torch.stack(outs).cpu().numpy(), torch.stack(counts).cpu().numpy()
    plan = stream_slots_plan(flags, chunk)
    assert (counts == np.array([[hi - lo for (_, lo, hi, _) in row] for row in plan])).all()
    sess = sessions(flags)
    by_start = {}
    for b, s0, s1 in sess:
        by_start.setdefault(s0, []).append((b, s1))
    checked = 0
    for s0, members in sorted(by_start.items()):
        rows = [b for b, _ in members]
        last = max(s1 for _, s1 in members)
        grp = rt.stream_open(len(rows), chunk)
        for s in range(s0, last + 1):
            ref = rt.stream_step(grp, x[rows, s * chunk:(s + 1) * chunk].contiguous()).cpu().numpy()
            for i, (b, s1) in enumerate(members):
                if s <= s1:
                    n = int(counts[s, b])
                    assert n == ref.shape[1] and outs[s, b, :n].tobytes() == ref[i].tobytes(), (s0, s, b)
                    checked += n
    pick = [sess[i] for i in np.linspace(0, len(sess) - 1, 16).astype(int)]
    for b, s0, s1 in pick:
        one = rt.stream_open(1, chunk)
        for s in range(s0, s1 + 1):
            ref = rt.stream_step(one, x[b:b + 1, s * chunk:(s + 1) * chunk].contiguous()).cpu().numpy()[0]
            assert outs[s, b, :int(counts[s, b])].tobytes() == ref.tobytes(), (b, s0, s)
    print(f"named size: {len(sess)} sessions in {len(by_start)} start groups, {checked} frames bitwise against lockstep groups, 16 against B = 1")
