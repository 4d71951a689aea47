"""GPU tests (-m gpu) of the log-mel slot pool (uvad_window_slots_*, VadRuntime.window_slots_*): B slots in lockstep, each holding at most
one session that starts and ends on its own flag bits.

  identity    each session's emitted frames, concatenated, are those of a B = 1 uvad_window_step stream opened at its start and fed the
              same chunks; its END step's flush is rows [Tw - L, Tw) of uvad_classify on that stream's features tap.  Bit for bit in
              GEMM modes 0 and 2 with a pinned recurrent tile, to 1e-5 in modes 1 and 3
  isolation   NaN / Inf / 1e30 in idle slots' chunk rows change no output bit; idle slots count 0
  one graph   the whole schedule, warm-ups and session changes included, replays from one captured graph (also on an idle GPU)
  plus the refusals and the named size (512 slots x 20 ms, W 500, L 50, sessions of U(2, 30) s restarting throughout).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG, E_STATE, E_WORKSPACE = -1, -3, -4      # include/uvad.h
TOL = 1e-5


def _model(F=64, scale=2.0):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=F)
    m.build()
    seed_weights(m, 1234, scale)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type="povey"))
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


def _schedule(B, steps, seed):
    """Flags (steps, B): slot 0 one long session; slot 1 one-chunk sessions; slot 2 a short session ended early; slot 3 restarted while
    busy and ended late; slots 4 .. B - 2 random churn (restarts, ends, one-chunk sessions); slot B - 1 idle throughout."""
    rng = np.random.default_rng(seed)
    f = np.zeros((steps, B), np.uint8)
    f[0, 0] = 1
    f[5, 1] = f[steps // 2, 1] = 3
    f[3, 2], f[8, 2] = 1, 2
    f[2, 3], f[10, 3], f[steps - 5, 3] = 1, 1, 2
    for b in range(4, B - 1):
        live = False
        for s in range(1 + b, steps):
            r = rng.random()
            if not live and r < 0.12:
                f[s, b] = 3 if rng.random() < 0.15 else 1
                live = f[s, b] == 1
            elif live and r < 0.03:
                f[s, b] = 1                                   # START on a busy slot
            elif live and r < 0.07:
                f[s, b], live = 2, False
    return f


def _pcm(B, steps, chunk, seed):
    from uvad_amd.synth import synth_pcm
    return torch.from_numpy(synth_pcm(B, steps * chunk, seed=seed)).to(DEV)


def _run_pool(rt, x, flags, chunk, W, L, graphs=False, sync=False, poison=None):
    """Every step of a slot pool over x (B, steps * chunk) -> [(logits (B, L + kmax), counts (B,))] (host copies)."""
    steps, B = flags.shape
    st = rt.window_slots_open(B, chunk, window=W, lookahead=L, graphs=graphs)
    live = np.zeros(B, bool)
    out = []
    for s in range(steps):
        xs = x[:, s * chunk:(s + 1) * chunk].clone()
        live[flags[s] & 1 == 1] = True
        if poison is not None:
            xs[torch.from_numpy(~live).to(DEV)] = poison
        if sync:
            torch.cuda.synchronize()
        fl = flags[s]
        lg, cnt = rt.window_slots_step(st, xs, start=fl & 1 == 1, end=fl & 2 == 2) if fl.any() else rt.window_slots_step(st, xs)
        out.append((lg.cpu().clone(), cnt.cpu().clone()))
        live[fl & 2 == 2] = False
    return out, st


def _sessions(flags):
    """[(slot, first step, last step, ended)] of a schedule."""
    steps, B = flags.shape
    out = []
    for b in range(B):
        s0 = None
        for s in range(steps):
            if flags[s, b] & 1:
                if s0 is not None:
                    out.append((b, s0, s - 1, False))
                s0 = s
            if flags[s, b] & 2 and s0 is not None:
                out.append((b, s0, s, True))
                s0 = None
        if s0 is not None:
            out.append((b, s0, steps - 1, False))
    return out


def _reference(rt, x, b, s0, s1, ended, chunk, W, L):
    """A B = 1 window stream over slot b's chunks s0 .. s1: its emitted logits, with the flush of an END step from classify on its tap."""
    st = rt.window_stream_open(1, chunk, window=W, lookahead=L)
    parts = []
    for s in range(s0, s1 + 1):
        lg = rt.window_stream_step(st, x[b:b + 1, s * chunk:(s + 1) * chunk].contiguous()).clone()
        parts.append(lg[0])
    if ended and st["frames"]:
        feats = rt.window_features(st)
        Tw = feats.shape[1]
        ref, _ = rt.classify(feats)
        flush = min(L, st["frames"])
        parts.append(ref[0, Tw - flush:Tw].clone())
    return torch.cat(parts).cpu() if parts else torch.zeros(0)


def _pool_session(out, b, s0, s1):
    return torch.cat([out[s][0][b, :int(out[s][1][b])] for s in range(s0, s1 + 1)])


def _check_counts(out, flags, chunk, W, L):
    from uvad_amd.runtime import window_slots_plan
    plan = window_slots_plan(flags, chunk, W, L)
    for s, (_, cnt) in enumerate(out):
        want = [hi - lo for (_, lo, hi, _) in plan[s]]
        assert cnt.tolist() == want, (s, cnt.tolist(), want)
    return plan


@pytest.mark.parametrize("mode", ["f32", "f16p_stream"])
@pytest.mark.parametrize("chunk", [320, 250, 1600])
@pytest.mark.parametrize("L", [0, 7, 50])
def test_every_session_is_its_single_feed_stream_bit_for_bit(L, chunk, mode):
    B, W = 8, 64                     # L + chunk // 160 + 1 <= W for every (L, chunk)
    steps = 90 if chunk != 1600 else 40
    m, rt = _model()
    rt.set_gemm_mode(mode)
    rt.set_recurrent_tile(4)
    flags = _schedule(B, steps, seed=chunk + L)
    x = _pcm(B, steps, chunk, seed=500 + chunk)
    out, _ = _run_pool(rt, x, flags, chunk, W, L)
    plan = _check_counts(out, flags, chunk, W, L)
    assert all(plan[s][B - 1][0] == -1 and int(out[s][1][B - 1]) == 0 for s in range(steps))
    sess = _sessions(flags)
    kinds = {"one-chunk": 0, "early end": 0, "late end": 0, "restart": 0}
    for b, s0, s1, ended in sess:
        got = _pool_session(out, b, s0, s1)
        want = _reference(rt, x, b, s0, s1, ended, chunk, W, L)
        assert got.shape == want.shape, (b, s0, s1, ended, got.shape, want.shape)
        assert torch.equal(got, want), (b, s0, s1, ended, float((got - want).abs().max()))
        e = plan[s1][b][3]
        kinds["one-chunk"] += s0 == s1
        kinds["early end"] += ended and e < W
        kinds["late end"] += ended and e >= W
        kinds["restart"] += not ended and s1 < steps - 1
    print(f"{mode} chunk {chunk} L {L}: {len(sess)} sessions {kinds}")
    assert all(v > 0 for v in kinds.values()), kinds


@pytest.mark.parametrize("mode", ["f16p", "f16p3"])
def test_modes_with_launch_size_dependent_kernels_agree_to_rounding(mode):
    B, W, L, chunk, steps = 8, 60, 7, 320, 90
    m, rt = _model()
    rt.set_gemm_mode(mode)
    flags = _schedule(B, steps, seed=77)
    x = _pcm(B, steps, chunk, seed=501)
    out, _ = _run_pool(rt, x, flags, chunk, W, L)
    _check_counts(out, flags, chunk, W, L)
    worst = 0.0
    for b, s0, s1, ended in _sessions(flags):
        got, want = _pool_session(out, b, s0, s1), _reference(rt, x, b, s0, s1, ended, chunk, W, L)
        assert got.shape == want.shape
        if got.numel():
            worst = max(worst, float((got - want).abs().max()))
    print(f"{mode}: worst |pool - single feed| = {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), 1e30])
def test_idle_slots_chunk_rows_are_never_read(poison):
    B, W, L, chunk, steps = 8, 60, 7, 320, 70
    m, rt = _model()
    flags = _schedule(B, steps, seed=78)
    x = _pcm(B, steps, chunk, seed=502)
    clean, _ = _run_pool(rt, x, flags, chunk, W, L, poison=0.0)
    dirty, _ = _run_pool(rt, x, flags, chunk, W, L, poison=poison)
    live = np.zeros(B, bool)
    for s in range(steps):
        live[flags[s] & 1 == 1] = True
        (a, ca), (b, cb) = clean[s], dirty[s]
        assert torch.equal(ca, cb)
        assert all(int(cb[i]) == 0 for i in range(B) if not live[i])
        for i in range(B):
            assert torch.equal(a[i, :int(ca[i])], b[i, :int(cb[i])]), (s, i)
        live[flags[s] & 2 == 2] = False


@pytest.mark.parametrize("sync", [False, True])
def test_one_captured_graph_replays_the_whole_schedule(sync):
    """Warm-ups, starts, restarts and ends all replay from the graph captured on the first step; sync: a device synchronise before
    every step, so each replay starts on an idle GPU."""
    B, W, L, chunk, steps = 8, 60, 7, 320, 90
    m, rt = _model()
    rt.set_gemm_mode("f16p")
    flags = _schedule(B, steps, seed=79)
    x = _pcm(B, steps, chunk, seed=503)
    eager, _ = _run_pool(rt, x, flags, chunk, W, L)
    replay, st = _run_pool(rt, x, flags, chunk, W, L, graphs=True, sync=sync)
    assert st["graphs"] == 1
    bad = [s for s in range(steps) if not torch.equal(eager[s][1], replay[s][1]) or
           any(not torch.equal(eager[s][0][i, :int(eager[s][1][i])], replay[s][0][i, :int(replay[s][1][i])]) for i in range(B))]
    print(f"sync={sync}: 1 graph, {steps} steps, differing from eager: {bad[:10]}")
    assert not bad
    assert rt.time_chunks() == 1


def test_window_slots_refusals():
    from uvad_amd.runtime import VadRuntime
    m, rt = _model()
    lib, ctx = rt.lib, rt.ctx
    B, chunk, W, L = 4, 320, 40, 7
    kmax = chunk // 160 + 1
    st = torch.empty(int(lib.uvad_window_slots_state_bytes(ctx, B, W)), dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(lib.uvad_window_slots_workspace_bytes(ctx, B, chunk, W)), dtype=torch.uint8, device=DEV)
    x = torch.zeros(B, chunk, device=DEV)
    out = torch.full((B, L + kmax), -7.0, device=DEV)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    flags = torch.ones(B, dtype=torch.uint8, device=DEV)
    s = rt._stream()

    def step(b=B, ch=chunk, ld=L + kmax, wsb=None, state=st, counts=cnt):
        return lib.uvad_window_slots_step(ctx, x.data_ptr(), flags.data_ptr(), b, ch, state.data_ptr(), out.data_ptr(), None, ld,
                                          counts.data_ptr() if counts is not None else None, ws.data_ptr(),
                                          ws.numel() if wsb is None else wsb, s)

    assert step() == E_STATE                                   # never reset
    assert lib.uvad_window_slots_reset(ctx, st.data_ptr(), B, 119, W, L, s) == E_ARG     # chunk < (400 - 160) / 2
    assert lib.uvad_window_slots_reset(ctx, st.data_ptr(), B, chunk, W, W - 2, s) == E_ARG   # L + kmax > W
    assert lib.uvad_window_slots_reset(ctx, st.data_ptr(), B, chunk, W, W, s) == E_ARG
    assert lib.uvad_window_slots_reset(ctx, st.data_ptr(), B, chunk, W, L, s) == 0
    torch.cuda.synchronize()
    assert step(b=B + 1) == E_ARG
    assert step(ch=chunk - 1) == E_ARG
    assert step(ld=L + kmax - 1) == E_ARG
    assert step(counts=None) == E_ARG
    assert step(wsb=ws.numel() - 1) == E_WORKSPACE
    torch.cuda.synchronize()
    assert int((cnt != -7).sum()) == 0 and bool((out == -7.0).all())   # nothing was enqueued
    f = torch.empty((B, W, 64), device=DEV)
    tw = torch.empty(B, dtype=torch.int32, device=DEV)
    assert lib.uvad_window_slots_features(ctx, st.data_ptr(), B + 1, f.data_ptr(), tw.data_ptr(), s) == E_ARG
    assert step() == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [0] * B                                       # a first chunk of 320 samples: one frame, L = 7 held back
    # a context without a model: the configuration is missing
    from uvad_amd.features import FbankConfig
    bare = VadRuntime(DEV, fbank=FbankConfig(num_filters=64))
    assert bare.lib.uvad_window_slots_state_bytes(bare.ctx, B, W) == 0
    assert bare.lib.uvad_window_slots_reset(bare.ctx, st.data_ptr(), B, chunk, W, L, s) == E_STATE


def test_named_size_512_slots_20ms_window_500_lookahead_50_under_churn():
    """512 slots x 320 samples, W = 500, L = 50; sessions of seeded U(2, 30) s lengths restart throughout (churn never stops).  Eight
    sessions spread over the run equal their B = 1 streams bit for bit (mode f16p_stream, tile 4); every count equals the plan."""
    from uvad_amd.runtime import window_slots_plan
    from uvad_amd.synth import synth_pcm
    B, chunk, W, L, steps = 512, 320, 500, 50, 1600
    m, rt = _model()
    rt.set_gemm_mode("f16p_stream")
    rt.set_recurrent_tile(4)
    rng = np.random.default_rng(512)
    flags = np.zeros((steps, B), np.uint8)
    for b in range(B):
        s = int(rng.integers(0, 150))
        while s < steps:
            n = int(rng.uniform(2, 30) * 50)
            flags[s, b] |= 1
            if s + n - 1 < steps:
                flags[s + n - 1, b] |= 2
            s += n + int(rng.integers(0, 20))
    base = torch.from_numpy(synth_pcm(B, 80 * chunk, seed=512)).to(DEV)

    def chunk_at(s, rows=slice(None)):
        j = s % 80
        return base[rows, j * chunk:(j + 1) * chunk]

    st = rt.window_slots_open(B, chunk, window=W, lookahead=L, graphs=True)
    plan = window_slots_plan(flags, chunk, W, L)
    sess = [t for t in _sessions(flags) if t[3] and t[2] - t[1] < 700]
    pick = [sess[i] for i in np.linspace(0, len(sess) - 1, 8).astype(int)]
    keep = {}
    counts = []
    for s in range(steps):
        fl = flags[s]
        lg, cnt = rt.window_slots_step(st, chunk_at(s), start=fl & 1 == 1, end=fl & 2 == 2)
        counts.append(cnt.clone())
        for b, s0, s1, _ in pick:
            if s0 <= s <= s1:
                keep.setdefault((b, s0), []).append(lg[b].clone())
    counts = torch.stack(counts).cpu().numpy()
    want = np.array([[hi - lo for (_, lo, hi, _) in row] for row in plan])
    assert (counts == want).all()
    assert st["graphs"] == 1
    for b, s0, s1, _ in pick:
        got = torch.cat([keep[(b, s0)][s - s0][:int(counts[s, b])] for s in range(s0, s1 + 1)]).cpu()
        ref = rt.window_stream_open(1, chunk, window=W, lookahead=L)
        parts = [rt.window_stream_step(ref, chunk_at(s, slice(b, b + 1)).contiguous())[0].clone() for s in range(s0, s1 + 1)]
        feats = rt.window_features(ref)
        lgf, _ = rt.classify(feats)
        parts.append(lgf[0, feats.shape[1] - min(L, ref["frames"]):].clone())
        want_b = torch.cat(parts).cpu()
        assert torch.equal(got, want_b), (b, s0, s1, float((got - want_b).abs().max()))
    starts = int((flags & 1).sum())
    print(f"named size: {steps} steps, {starts} session starts, {int(counts.sum())} frames emitted, 8 sessions bitwise")
