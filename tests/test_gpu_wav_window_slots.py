"""GPU tests (-m gpu) of the waveform slot pool (uvad_window_wav_slots_*, VadRuntime.wav_window_slots_*): the SincNet PyanNet served by B
slots in lockstep, each holding at most one session that starts and ends on its own flag bits; f32 and int16 feeds.

  identity    each session's emitted frames, concatenated, are those of a B = 1 uvad_window_wav_step[_i16] stream opened at its start and
              fed the same chunks; its END step's flush is rows [Tw - L, Tw) of uvad_classify on that stream's SincNet tap.  Bit for bit in
              GEMM modes 0 and 2 (exact-f32 SincNet in both runs) with a pinned recurrent tile
  isolation   NaN / Inf / 1e30 (f32) or any int16 in idle slots' chunk rows change no output bit; idle slots count 0
  one graph   the whole schedule replays from one captured graph (also on an idle GPU)
  plus the refusals and the named size (512 int16 slots x 20 ms, W 293, L 30, sessions of U(2, 30) s restarting throughout).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG, E_STATE, E_WORKSPACE = -1, -3, -4      # include/uvad.h


def _model(seed=11, scale=2.0):
    """Seeded PyanNet: default-initialised SincNet (torch-default conv weights under `seed`), seeded classifier."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    torch.manual_seed(seed)
    m = uvad_amd.PyanNet()
    m.build()
    seed_weights(m, 1234, scale)
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


def _pcm(B, steps, chunk, seed, i16):
    from uvad_amd.synth import synth_pcm
    x = synth_pcm(B, steps * chunk, seed=seed)
    if i16:
        return torch.from_numpy(np.round(x * 32767.0).astype(np.int16)).to(DEV)
    return torch.from_numpy(x).to(DEV)


def _run_pool(rt, x, flags, chunk, W, L, graphs=False, sync=False, poison=None):
    """Every step of a waveform slot pool over x (B, steps * chunk) -> [(logits (B, L + kmax), counts (B,))] (host copies)."""
    steps, B = flags.shape
    st = rt.wav_window_slots_open(B, chunk, window=W, lookahead=L, graphs=graphs, dtype=x.dtype)
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
        lg, cnt = rt.wav_window_slots_step(st, xs, start=fl & 1 == 1, end=fl & 2 == 2) if fl.any() else rt.wav_window_slots_step(st, xs)
        out.append((lg.cpu().clone(), cnt.cpu().clone()))
        live[fl & 2 == 2] = False
    return out, st


def _reference(rt, x, b, s0, s1, ended, chunk, W, L):
    """A B = 1 waveform window stream over slot b's chunks s0 .. s1: its emitted logits, with the flush of an END step from classify on
    its SincNet tap."""
    st = rt.wav_window_stream_open(1, chunk, window=W, lookahead=L, dtype=x.dtype)
    parts = []
    for s in range(s0, s1 + 1):
        parts.append(rt.wav_window_stream_step(st, x[b:b + 1, s * chunk:(s + 1) * chunk].contiguous())[0].clone())
    if ended and st["frames"]:
        feats = rt.wav_window_features(st)
        Tw = feats.shape[1]
        ref, _ = rt.classify(feats)
        parts.append(ref[0, Tw - min(L, st["frames"]):Tw].clone())
    return torch.cat(parts).cpu()


def _pool_session(out, b, s0, s1):
    return torch.cat([out[s][0][b, :int(out[s][1][b])] for s in range(s0, s1 + 1)])


def _check_counts(rt, out, flags, chunk, W, L):
    from uvad_amd.runtime import wav_window_slots_plan
    J, R = rt.wav_window_geometry()
    plan = wav_window_slots_plan(flags, chunk, W, L, J, R)
    for s, (_, cnt) in enumerate(out):
        want = [hi - lo for (_, lo, hi, _) in plan[s]]
        assert cnt.tolist() == want, (s, cnt.tolist(), want)
    return plan


@pytest.mark.parametrize("mode", ["f32", "f16p_stream"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
@pytest.mark.parametrize("chunk", [320, 250, 1600])
@pytest.mark.parametrize("L", [0, 7, 50])
def test_every_session_is_its_single_feed_stream_bit_for_bit(L, chunk, dtype, mode):
    B, W = 8, 60
    steps = 90 if chunk != 1600 else 40
    i16 = dtype == torch.int16
    m, rt = _model()
    rt.set_gemm_mode(mode)
    rt.set_recurrent_tile(4)
    flags = _schedule(B, steps, seed=chunk + L + i16)
    x = _pcm(B, steps, chunk, seed=600 + chunk, i16=i16)
    out, _ = _run_pool(rt, x, flags, chunk, W, L)
    assert rt.sincnet_form() == "f32"
    plan = _check_counts(rt, out, flags, chunk, W, L)
    assert all(plan[s][B - 1][0] == -1 and int(out[s][1][B - 1]) == 0 for s in range(steps))
    kinds = {"one-chunk": 0, "early end": 0, "late end": 0, "restart": 0}
    sess = _sessions(flags)
    for b, s0, s1, ended in sess:
        got = _pool_session(out, b, s0, s1)
        want = _reference(rt, x, b, s0, s1, ended, chunk, W, L)
        assert rt.sincnet_form() == "f32"
        assert got.shape == want.shape, (b, s0, s1, ended, got.shape, want.shape)
        assert torch.equal(got, want), (b, s0, s1, ended, float((got - want).abs().max()))
        e = plan[s1][b][3]
        kinds["one-chunk"] += s0 == s1
        kinds["early end"] += ended and e < W
        kinds["late end"] += ended and e >= W
        kinds["restart"] += not ended and s1 < steps - 1
    print(f"{mode} {str(dtype)[6:]} chunk {chunk} L {L}: {len(sess)} sessions {kinds}")
    assert all(v > 0 for v in kinds.values()), kinds


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), 1e30, "i16"])
def test_idle_slots_chunk_rows_are_never_read(poison):
    B, W, L, chunk, steps = 8, 60, 7, 320, 80
    i16 = poison == "i16"
    m, rt = _model()
    flags = _schedule(B, steps, seed=88)
    x = _pcm(B, steps, chunk, seed=602, i16=i16)
    clean, _ = _run_pool(rt, x, flags, chunk, W, L, poison=0)
    dirty, _ = _run_pool(rt, x, flags, chunk, W, L, poison=-32768 if i16 else poison)
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
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_one_captured_graph_replays_the_whole_schedule(dtype, sync):
    B, W, L, chunk, steps = 8, 60, 7, 320, 90
    m, rt = _model()
    rt.set_gemm_mode("f16p")
    flags = _schedule(B, steps, seed=89)
    x = _pcm(B, steps, chunk, seed=603, i16=dtype == torch.int16)
    eager, _ = _run_pool(rt, x, flags, chunk, W, L)
    replay, st = _run_pool(rt, x, flags, chunk, W, L, graphs=True, sync=sync)
    assert st["graphs"] == 1
    bad = [s for s in range(steps) if not torch.equal(eager[s][1], replay[s][1]) or
           any(not torch.equal(eager[s][0][i, :int(eager[s][1][i])], replay[s][0][i, :int(replay[s][1][i])]) for i in range(B))]
    print(f"{str(dtype)[6:]} sync={sync}: 1 graph, {steps} steps, differing from eager: {bad[:10]}")
    assert not bad


def test_wav_window_slots_refusals():
    m, rt = _model()
    lib, ctx = rt.lib, rt.ctx
    B, chunk, W, L = 4, 320, 40, 7
    kmax = -(-chunk // 270)
    st = torch.empty(int(lib.uvad_window_wav_slots_state_bytes(ctx, B, W, 1)), dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(lib.uvad_window_wav_slots_workspace_bytes(ctx, B, chunk, W)), dtype=torch.uint8, device=DEV)
    x = torch.zeros(B, chunk, dtype=torch.int16, device=DEV)
    out = torch.full((B, L + kmax), -7.0, device=DEV)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    flags = torch.ones(B, dtype=torch.uint8, device=DEV)
    s = rt._stream()

    def step(fn=lib.uvad_window_wav_slots_step_i16, b=B, ch=chunk, ld=L + kmax, wsb=None, counts=cnt):
        return fn(ctx, x.data_ptr(), flags.data_ptr(), b, ch, st.data_ptr(), out.data_ptr(), None, ld,
                  counts.data_ptr() if counts is not None else None, ws.data_ptr(), ws.numel() if wsb is None else wsb, s)

    assert step() == E_STATE                                   # never reset
    assert lib.uvad_window_wav_slots_reset(ctx, st.data_ptr(), B, 271 * 40, W, 0, 1, s) == E_ARG   # ceil(chunk / J) > W
    assert lib.uvad_window_wav_slots_reset(ctx, st.data_ptr(), B, chunk, W, W - 1, 1, s) == E_ARG  # L + kmax > W
    assert lib.uvad_window_wav_slots_reset(ctx, st.data_ptr(), B, chunk, W, L, 2, s) == E_ARG
    assert lib.uvad_window_wav_slots_reset(ctx, st.data_ptr(), B, chunk, W, L, 1, s) == 0
    torch.cuda.synchronize()
    assert step(fn=lib.uvad_window_wav_slots_step) == E_ARG  # f32 step on an int16 pool
    assert step(b=B + 1) == E_ARG
    assert step(ch=chunk + 1) == E_ARG
    assert step(ld=L + kmax - 1) == E_ARG
    assert step(counts=None) == E_ARG
    assert step(wsb=ws.numel() - 1) == E_WORKSPACE
    torch.cuda.synchronize()
    assert int((cnt != -7).sum()) == 0 and bool((out == -7.0).all())   # nothing was enqueued
    assert step() == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [0] * B                                       # 320 samples: no frame yet
    # a context without a SincNet configuration
    import uvad_amd
    m2 = uvad_amd.PyanNet2(encoding_dim=64)
    m2.build()
    m2 = m2.to(DEV).eval()
    rt2 = m2.runtime(DEV)
    assert rt2.lib.uvad_window_wav_slots_state_bytes(rt2.ctx, B, W, 1) == 0
    assert rt2.lib.uvad_window_wav_slots_reset(rt2.ctx, st.data_ptr(), B, chunk, W, L, 1, s) == E_STATE


def test_named_size_512_int16_slots_20ms_window_293_lookahead_30_under_churn():
    """512 int16 slots x 320 samples, W = 293, L = 30; sessions of seeded U(2, 30) s lengths restart throughout.  Eight sessions spread
    over the run equal their B = 1 streams bit for bit (mode f16p_stream, tile 4); every count equals the plan."""
    from uvad_amd.runtime import wav_window_slots_plan
    from uvad_amd.synth import synth_pcm
    B, chunk, W, L, steps = 512, 320, 293, 30, 1600
    m, rt = _model()
    rt.set_gemm_mode("f16p_stream")
    rt.set_recurrent_tile(4)
    rng = np.random.default_rng(513)
    flags = np.zeros((steps, B), np.uint8)
    for b in range(B):
        s = int(rng.integers(0, 150))
        while s < steps:
            n = int(rng.uniform(2, 30) * 50)
            flags[s, b] |= 1
            if s + n - 1 < steps:
                flags[s + n - 1, b] |= 2
            s += n + int(rng.integers(0, 20))
    base = torch.from_numpy(np.round(synth_pcm(B, 80 * chunk, seed=513) * 32767.0).astype(np.int16)).to(DEV)

    def chunk_at(s, rows=slice(None)):
        j = s % 80
        return base[rows, j * chunk:(j + 1) * chunk]

    J, R = rt.wav_window_geometry()
    st = rt.wav_window_slots_open(B, chunk, window=W, lookahead=L, graphs=True, dtype=torch.int16)
    plan = wav_window_slots_plan(flags, chunk, W, L, J, R)
    sess = [t for t in _sessions(flags) if t[3] and t[2] - t[1] < 700]
    pick = [sess[i] for i in np.linspace(0, len(sess) - 1, 8).astype(int)]
    keep = {}
    counts = []
    for s in range(steps):
        fl = flags[s]
        lg, cnt = rt.wav_window_slots_step(st, chunk_at(s).contiguous(), start=fl & 1 == 1, end=fl & 2 == 2)
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
        ref = rt.wav_window_stream_open(1, chunk, window=W, lookahead=L, dtype=torch.int16)
        parts = [rt.wav_window_stream_step(ref, chunk_at(s, slice(b, b + 1)).contiguous())[0].clone() for s in range(s0, s1 + 1)]
        feats = rt.wav_window_features(ref)
        lgf, _ = rt.classify(feats)
        parts.append(lgf[0, feats.shape[1] - min(L, ref["frames"]):].clone())
        want_b = torch.cat(parts).cpu()
        assert torch.equal(got, want_b), (b, s0, s1, float((got - want_b).abs().max()))
    print(f"named size: {steps} steps, {int((flags & 1).sum())} session starts, {int(counts.sum())} frames emitted, 8 sessions bitwise")
