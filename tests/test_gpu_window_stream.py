"""GPU tests (-m gpu) of windowed streaming (uvad_window_*, VadRuntime.window_stream_*): a bidirectional PyanNet2 served live by
re-running it from zero state over the last W frames, emitting each frame L frames behind the newest complete one.

  plumbing   every emitted logit is bit-identical to its row in uvad_classify on the step's window (the uvad_window_features tap) at
             the same (B, Tw) and GEMM mode, and the tap equals the offline features of the whole signal
  semantics  emitted logits = uvad_classify on windows sliced from the offline features, to LOGIT_TOL (weights x2)
  truth      at weights x4 the GPU is no further from the float64 truth than the fp32 CPU path (1.5 x on the rms)
  plus the causal cross-check against uvad_stream_step, graph replay, refusals and the named size (512 feeds, 20 ms, W 500, L 50).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
FEAT_TOL = 5e-4


def _model(F, scale=2.0, bidirectional=True, window_type="povey"):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    m = uvad_amd.PyanNet2(lstm={"bidirectional": bidirectional}, encoding_dim=F)
    m.build()
    seed_weights(m, 1234, scale)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type=window_type))
    m = m.to(dev).eval()
    return m, m.runtime(dev)


def _run(rt, x, chunk, W, L, graphs=False, tap=None):
    """Every step of a window stream group over x (B, S): [(schedule row, logits (B, k))]; tap(state, row, logits) after each step."""
    from uvad_amd.runtime import window_schedule
    B, S = x.shape
    steps = S // chunk
    sched = window_schedule(steps, chunk, W, L)
    st = rt.window_stream_open(B, chunk, window=W, lookahead=L, graphs=graphs)
    out = []
    for i in range(steps):
        lg = rt.window_stream_step(st, x[:, i * chunk:(i + 1) * chunk].contiguous()).clone()
        assert lg.shape == (B, sched[i][0])
        if tap:
            tap(st, sched[i], lg)
        out.append((sched[i], lg))
    return out, st


@pytest.mark.parametrize("mode", ["f32", "f16p", "f16p3"])
def test_window_steps_are_bit_identical_to_classify_on_the_feature_tap(mode):
    """Exact plumbing over a run that crosses from warm-up into steady state (W = 64 frames, 1.5 s): the emitted rows are the bits
    uvad_classify gives on the tapped window at the same (B, Tw), and the tap is the offline feature stream of the whole signal."""
    from uvad_amd.synth import synth_pcm
    B, F, chunk, W, L = 5, 64, 320, 64, 7
    m, rt = _model(F)
    rt.set_gemm_mode(mode)
    x = torch.from_numpy(synth_pcm(B, 24000, seed=301)).cuda()
    offline = rt.fbank(x)
    worst = [0.0]
    seen = set()

    def tap(st, row, lg):
        k, lo, hi, e0, e1 = row
        feats = rt.window_features(st)
        assert feats.shape == (B, hi - lo, F)
        worst[0] = max(worst[0], float((feats - offline[:, lo:hi]).abs().max()))
        if k:
            ref, _ = rt.classify(feats)
            assert torch.equal(lg, ref[:, e0 - lo:e1 - lo]), (row, float((lg - ref[:, e0 - lo:e1 - lo]).abs().max()))
        seen.add(hi - lo)

    out, _ = _run(rt, x, chunk, W, L, tap=tap)
    print(f"mode {mode}: {len(out)} steps, window sizes {min(seen)}..{max(seen)}, tap vs offline features {worst[0]:.2e}")
    assert max(seen) == W and min(seen) < W
    assert worst[0] < FEAT_TOL
    assert rt.time_chunks() == 1


@pytest.mark.parametrize("mode", ["f32", "f16p", "f16p3"])
@pytest.mark.parametrize("chunk", [320, 250, 1600])
@pytest.mark.parametrize("L", [0, 7, 50])
def test_window_logits_equal_classify_on_offline_windows(L, chunk, mode):
    """Semantics: frame t emitted after a step with e complete frames is row t of the model run from zero state over the offline
    features [max(0, e - W), e), to LOGIT_TOL at weights x2 (W = 120 frames, 2.5 s: warm-up and steady state)."""
    from uvad_amd.synth import synth_pcm
    B, F, W = 6, 64, 120
    m, rt = _model(F)
    rt.set_gemm_mode(mode)
    S = 40000 // chunk * chunk
    x = torch.from_numpy(synth_pcm(B, S, seed=302 + chunk)).cuda()
    offline = rt.fbank(x)
    out, _ = _run(rt, x, chunk, W, L)
    err, n = 0.0, 0
    for (k, lo, hi, e0, e1), lg in out:
        if not k:
            continue
        ref, _ = rt.classify(offline[:, lo:hi].contiguous())
        err = max(err, float((lg - ref[:, e0 - lo:e1 - lo]).abs().max()))
        n += k
    last = out[-1][0]
    print(f"L={L} chunk={chunk} {mode}: {n} frames emitted, max |window - offline window| = {err:.2e}")
    assert last[2] - last[1] == W and n == last[4] == last[2] - L
    assert err < LOGIT_TOL


def test_window_logits_no_further_from_float64_truth_than_the_cpu_path():
    """Truth (weights x4, the near-chaotic network): on a few feeds and steps the emitted logits are no further from the float64
    truth (float64 features -> float64 network over the same window) than the reference's fp32 CPU path is (1.5 x on the rms)."""
    from uvad_amd.synth import synth_pcm
    from oracle import c_oracle as co, parity_stats as ps, torch_ref as tr
    B, F, chunk, W, L = 4, 64, 320, 100, 7
    m, rt = _model(F, scale=4.0, window_type="hamming")
    pcm = synth_pcm(B, 32000, seed=303)
    out, _ = _run(rt, torch.from_numpy(pcm).cuda(), chunk, W, L)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    cfg = co.default_fbank_cfg(F)
    f64 = co.fbank_f64(pcm, cfg, co.window("hamming", 400), co.mel_banks(cfg))
    f32 = tr.torch_fbank(torch.from_numpy(pcm), tr.make_window("hamming", 400), tr.make_mel(F))
    cpu = tr.TorchPyanNet2(F)
    cpu.load_state_dict(sd)
    g, c, t = [], [], []
    picked = [r for r in out if r[0][0]][::6]
    for (k, lo, hi, e0, e1), lg in picked:
        g.append(lg.cpu().numpy())
        with torch.no_grad():
            c.append(cpu(f32[:, lo:hi])[0].numpy()[:, e0 - lo:e1 - lo])
        t.append(ps.truth_logits(sd, f64[:, lo:hi], F)[:, e0 - lo:e1 - lo])
    g, c, t = (np.concatenate(a, axis=1) for a in (g, c, t))
    sg, sc = ps.error_stats(g, t), ps.error_stats(c, t)
    print(f"{len(picked)} steps: " + ps.fmt("GPU vs f64 truth", sg))
    print(f"{len(picked)} steps: " + ps.fmt("CPU fp32 vs f64 truth", sc))
    assert sg["rms"] <= 1.5 * sc["rms"], (sg, sc)


def test_causal_model_with_zero_lookahead_equals_stream_step_during_warm_up():
    """A bidirectional = False model, L = 0: while e < W the window is the prefix [0, e), so the last rows are what the carried-state
    stream (uvad_stream_step) emits."""
    from uvad_amd.synth import synth_pcm
    B, F, chunk, W = 6, 64, 320, 300
    m, rt = _model(F, bidirectional=False)
    x = torch.from_numpy(synth_pcm(B, 32000, seed=304)).cuda()
    out, _ = _run(rt, x, chunk, W, 0)
    st = rt.stream_open(B, chunk)
    err, n = 0.0, 0
    for i, ((k, lo, hi, e0, e1), lg) in enumerate(out):
        ref = rt.stream_step(st, x[:, i * chunk:(i + 1) * chunk].contiguous())
        assert ref.shape == lg.shape
        if hi < W:
            err = max(err, float((lg - ref).abs().max()))
            n += k
    print(f"causal L = 0: {n} warm-up frames, max |window - stream| = {err:.2e}")
    assert n >= 190 and err < LOGIT_TOL


@pytest.mark.parametrize("chunk", [320, 250, 1600])
def test_graph_replay_is_bit_identical_and_settles_into_few_graphs(chunk):
    from math import gcd
    from uvad_amd.synth import synth_pcm
    B, F, W, L = 5, 64, 80, 7
    m, rt = _model(F)
    S = 48000 // chunk * chunk
    x = torch.from_numpy(synth_pcm(B, S, seed=305)).cuda()
    runs = {}
    for graphs in (False, True):
        out, st = _run(rt, x, chunk, W, L, graphs=graphs)
        runs[graphs] = torch.cat([lg for _, lg in out], dim=1)
        if graphs:
            bound = 2 * (chunk * 160 // gcd(chunk, 160)) // chunk   # parity x the chunk / shift cycle
            print(f"chunk {chunk}: {len(st['graphs'])} graphs for {len(out)} steps (bound {bound})")
            assert 1 <= len(st["graphs"]) <= bound
    assert runs[True].shape == runs[False].shape and torch.equal(runs[True], runs[False])
    assert rt.time_chunks() == 1


@pytest.mark.parametrize("mode", ["f16p", "f32"])
def test_graph_replay_on_an_idle_gpu_equals_eager_step_by_step(mode):
    """Every replayed step launched on an idle GPU (a device synchronise before each step): the replayed graphs' tile-queue counter
    resets must reach the persistent kernels' atomics.  With those resets as hipMemsetAsync blit nodes, one of the two graphs re-emitted
    the previous step's logits on every replay (its fused head found the queue exhausted)."""
    from uvad_amd.synth import synth_pcm
    B, F, chunk, W, L, steps = 5, 64, 320, 80, 7, 120
    m, rt = _model(F)
    rt.set_gemm_mode(mode)
    x = torch.from_numpy(synth_pcm(B, steps * chunk, seed=307)).cuda()
    eager, _ = _run(rt, x, chunk, W, L)
    st = rt.window_stream_open(B, chunk, window=W, lookahead=L, graphs=True)
    bad = []
    for i in range(steps):
        torch.cuda.synchronize()
        lg = rt.window_stream_step(st, x[:, i * chunk:(i + 1) * chunk].contiguous()).clone()
        if not torch.equal(lg, eager[i][1]):
            bad.append(i)
    print(f"{mode}: {len(st['graphs'])} graphs, {steps} steps, steps differing from eager: {bad[:10]}")
    assert len(st["graphs"]) == 2 and not bad


def test_window_refusals_and_bidirectional_reset():
    import uvad_amd
    from uvad_amd import _lib
    from uvad_amd.runtime import VadRuntime
    dev = torch.device("cuda:0")
    m, rt = _model(64)
    lib, ctx = rt.lib, rt.ctx
    B, chunk, W, L = 4, 320, 40, 7
    # the new ground: a bidirectional model resets (the carried-state stream still refuses it)
    st = rt.window_stream_open(B, chunk, window=W, lookahead=L)
    with pytest.raises(_lib.UvadError) as ei:
        rt.stream_open(B, chunk)
    assert ei.value.code == -5
    state, ws = st["state"], st["ws"]
    x = torch.zeros((B, chunk), device=dev)
    out = torch.empty((B, 8), device=dev)
    s = rt._stream()

    def step(state_ptr, ld=8, ws_bytes=None, chunk_=chunk):
        return lib.uvad_window_step(ctx, x.data_ptr(), B, chunk_, state_ptr, out.data_ptr(), None, ld, ws.data_ptr(),
                                    ws.numel() if ws_bytes is None else ws_bytes, s)

    def err(code, want, text):
        assert code == want, (code, lib.uvad_last_error(ctx))
        assert text in lib.uvad_last_error(ctx).decode()

    assert lib.uvad_window_reset(ctx, state.data_ptr(), B, 0, 0, s) == -1                        # W < 1
    assert b"window must be >= 1" in lib.uvad_last_error(ctx)
    assert lib.uvad_window_reset(ctx, state.data_ptr(), B, W, L, s) == 0
    err(step(state.data_ptr(), chunk_=160 * 33), -1, "exceeds the window")                       # L + kmax = 7 + 34 > 40
    other = torch.empty_like(state)
    err(step(other.data_ptr()), -3, "uvad_window_reset")                                          # unreset state
    err(step(state.data_ptr(), ws_bytes=ws.numel() - 1), -4, "workspace too small")
    # ld_out smaller than the k of this step: nothing is enqueued or counted, the next call with room succeeds
    k0 = C.c_int()
    key = C.c_int64()
    n = 0
    while True:
        assert lib.uvad_window_peek(ctx, state.data_ptr(), chunk, C.byref(k0), C.byref(key)) == 0
        if k0.value:
            break
        assert step(state.data_ptr()) == 0
        n += 1
    err(step(state.data_ptr(), ld=k0.value - 1), -1, "ld_out")
    assert step(state.data_ptr()) == k0.value
    torch.cuda.synchronize()
    # configurations the window stream does not take
    lstm = {"hidden_size": 128, "num_layers": 2, "bidirectional": True}
    lin = {"hidden_size": 128, "num_layers": 2}
    snip = VadRuntime(dev, uvad_amd.FbankConfig(num_filters=64, snip_edges=True), {"encoding_dim": 64, "lstm": lstm, "linear": lin})
    assert snip.lib.uvad_window_reset(snip.ctx, state.data_ptr(), B, W, L, s) == -5
    assert b"snip_edges" in snip.lib.uvad_last_error(snip.ctx)
    wrong = VadRuntime(dev, uvad_amd.FbankConfig(num_filters=64), {"encoding_dim": 80, "lstm": lstm, "linear": lin})
    assert wrong.lib.uvad_window_reset(wrong.ctx, state.data_ptr(), B, W, L, s) == -1
    assert b"n_mels != encoding_dim" in wrong.lib.uvad_last_error(wrong.ctx)
    snip.close()
    wrong.close()


def test_named_size_512_feeds_20ms_chunks_window_500_lookahead_50():
    """512 feeds x 320-sample chunks x 7 s (past the 5 s warm-up), W = 500, L = 50, bidirectional PyanNet2 (F = 80): every emitted
    frame of every feed against uvad_classify on the offline window to LOGIT_TOL, and 5 feeds end to end against the float64 truth."""
    from uvad_amd.synth import synth_pcm_device
    from oracle import c_oracle as co, parity_stats as ps
    B, F, chunk, W, L, S = 512, 80, 320, 500, 50, 16000 * 7
    m, rt = _model(F, window_type="hamming")
    dev = torch.device("cuda:0")
    x = synth_pcm_device(B, S, seed=306, device=dev)
    offline = rt.fbank(x)
    out, st = _run(rt, x, chunk, W, L)
    err, n = 0.0, 0
    sub = [0, 1, 255, 256, 511]
    picked = []
    for i, ((k, lo, hi, e0, e1), lg) in enumerate(out):
        if not k:
            continue
        ref, _ = rt.classify(offline[:, lo:hi].contiguous())
        err = max(err, float((lg - ref[:, e0 - lo:e1 - lo]).abs().max()))
        n += k
        if i % 25 == 0 or i == len(out) - 1:
            picked.append(((lo, hi, e0, e1), lg[sub].cpu().numpy()))
    last = out[-1][0]
    print(f"named size: {len(out)} steps, {n} frames per feed, max |window - offline window| = {err:.2e}")
    assert last[2] - last[1] == W and n == last[4] and all(r[0] == 2 for r, _ in out[30:])
    assert torch.isfinite(out[-1][1]).all() and err < LOGIT_TOL
    assert rt.time_chunks() == 1
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    cfg = co.default_fbank_cfg(F)
    f64 = co.fbank_f64(x[sub].cpu().numpy(), cfg, co.window("hamming", 400), co.mel_banks(cfg), threads=5)
    worst = 0.0
    for (lo, hi, e0, e1), lg in picked:
        t = ps.truth_logits(sd, f64[:, lo:hi], F)[:, e0 - lo:e1 - lo]
        worst = max(worst, float(np.abs(lg - t).max()))
    print(f"named size: 5 feeds x {len(picked)} steps vs the float64 truth {worst:.2e}")
    assert worst < 5e-4          # end to end from PCM: the fp32 and float64 feature stages differ by ~1e-4 in the log domain (weights x2)
