"""GPU tests (-m gpu) of the waveform model's windowed stream (uvad_window_wav_*, VadRuntime.wav_window_stream_*): a PyanNet (SincNet
front end + BiLSTM head) served live from raw PCM by re-running it from zero state over the last W frames, emitting each frame L
frames behind the newest complete one.

  plumbing   every emitted logit, warm-up included, is bit-identical to its row of uvad_forward_wav (_i16) on that window's samples at
             the same (B, S_w) and GEMM mode, time chunks 1; the features tap is uvad_sincnet on the same window, bit for bit
  truth      at weights x4 the emitted logits are no further from the float64 truth than the fp32 CPU path (1.5 x on rms and max)
  plus graph replay (also on an idle GPU), refusals and the named size (512 feeds, 20 ms, W 293, L 30).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REL = 1.5


def _model(seed=11, scale=4.0):
    """Seeded PyanNet: default-initialised SincNet (torch-default conv weights under `seed`), seeded classifier."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    torch.manual_seed(seed)
    m = uvad_amd.PyanNet()
    m.build()
    seed_weights(m, 1234, scale)
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


def _pair(seed=99, scale=4.0):
    """(torch-CPU SincNet, torch-CPU classifier, its state dict, uvad_amd.PyanNet with the same weights on the GPU)."""
    import uvad_amd
    from oracle import torch_ref as tr
    front = tr.seeded_sincnet(seed)
    csd = tr.seeded_state_dict(60, 128, 4, True, seed=4321, scale=scale)
    cls = tr.TorchPyanNet2(60, 128, 4, True)
    cls.load_state_dict(csd)
    m = uvad_amd.PyanNet()
    m.build()
    sd = dict(csd)
    fsd = front.state_dict()
    for k in ("wav_norm1d.weight", "wav_norm1d.bias"):
        sd["sincnet." + k] = fsd[k]
    sd["sincnet.conv1d.0.filterbank.low_hz_"] = fsd["low_hz_"]
    sd["sincnet.conv1d.0.filterbank.band_hz_"] = fsd["band_hz_"]
    for i in range(3):
        for p in ("weight", "bias"):
            sd[f"sincnet.norm1d.{i}.{p}"] = fsd[f"norm1d.{i}.{p}"]
    for i in range(2):
        for p in ("weight", "bias"):
            sd[f"sincnet.conv1d.{i + 1}.{p}"] = fsd[f"conv1d.{i}.{p}"]
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV).eval()
    return front, cls.eval(), csd, m


def _pcm(B, S, seed, i16):
    from uvad_amd.synth import synth_pcm
    x = synth_pcm(B, S, seed=seed)
    if i16:
        return torch.from_numpy(np.round(x * 32767.0).astype(np.int16)).to(DEV)
    return torch.from_numpy(x).to(DEV)


def _run(rt, x, chunk, W, L, graphs=False, tap=None, sync=False):
    """Every step of a waveform window stream group over x (B, S): [(schedule row, logits (B, k))]; tap(state, row, logits) after each."""
    from uvad_amd.runtime import wav_window_schedule
    B, S = x.shape
    J, R = rt.wav_window_geometry()
    steps = S // chunk
    sched = wav_window_schedule(steps, chunk, W, L, J, R)
    st = rt.wav_window_stream_open(B, chunk, window=W, lookahead=L, graphs=graphs, dtype=x.dtype)
    out = []
    for i in range(steps):
        if sync:
            torch.cuda.synchronize()
        lg = rt.wav_window_stream_step(st, x[:, i * chunk:(i + 1) * chunk].contiguous()).clone()
        assert lg.shape == (B, sched[i][0])
        if tap:
            tap(st, sched[i], lg)
        out.append((sched[i], lg))
    return out, st


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. bit identity with uvad_forward_wav on each window

@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
@pytest.mark.parametrize("mode", ["f32", "f16p", "f16p3"])
def test_emitted_rows_are_forward_wav_on_the_window_bit_for_bit(mode, dtype):
    """B = 7, W = 48 frames (~13 k samples), over chunks {160, 270, 320, 1600} x L {0, 7, 40}: every step's emitted rows are the bits of
    uvad_forward_wav (_i16) on that step's window samples at (B, S_w), warm-up included; the features tap is uvad_sincnet on the window."""
    B, W = 7, 48
    m, rt = _model()
    rt.set_gemm_mode(mode)
    rt.set_time_chunks(1)
    i16 = dtype == torch.int16
    x = _pcm(B, 20000, seed=401 + i16, i16=i16)
    form = "f32" if mode == "f32" else "f16p"
    for chunk in (160, 270, 320, 1600):
        for L in (0, 7, 40):
            seen, emitted = set(), 0

            def tap(st, row, lg):
                nonlocal emitted
                k, lo, hi, e0, e1, s0, s1 = row
                if hi == 0:
                    assert rt.wav_window_features(st).shape == (B, 0, 60)
                    return
                win = x[:, s0:s1].contiguous()
                assert rt.sincnet_num_frames(s1 - s0) == hi - lo
                feats = rt.wav_window_features(st)
                ref_f = rt.sincnet(win)
                assert torch.equal(feats, ref_f), (chunk, L, row)
                if k:
                    ref, _ = rt.forward_wav(win)
                    assert rt.sincnet_form() == form
                    assert torch.equal(lg, ref[:, e0 - lo:e1 - lo]), (chunk, L, row, float((lg - ref[:, e0 - lo:e1 - lo]).abs().max()))
                    emitted += k
                seen.add(hi - lo)

            out, st = _run(rt, x, chunk, W, L, tap=tap)
            last = out[-1][0]
            assert max(seen) == W and min(seen) < W
            assert emitted == last[4] == last[2] - L
            assert rt.time_chunks() == 1
            print(f"{mode} {str(dtype)[6:]} chunk {chunk} L {L}: {len(out)} steps, {emitted} frames per feed bit-identical")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. accuracy against the float64 truth

def test_emitted_logits_no_further_from_float64_truth_than_the_cpu_path():
    """Weights x4 (the near-chaotic classifier): on 4 feeds and a spread of steps, warm-up and steady state, the emitted logits are no
    further from the float64 truth (truth_sincnet -> truth_logits on each window) than the fp32 CPU path is (1.5 x on rms and max)."""
    from oracle import parity_stats as ps
    torch.set_num_threads(min(16, torch.get_num_threads()))
    front, cls, csd, m = _pair(scale=4.0)
    rt = m.runtime(DEV)
    B, chunk, W, L = 4, 320, 120, 7
    x = _pcm(B, 48000, seed=403, i16=False)
    out, _ = _run(rt, x, chunk, W, L)
    xc = x.cpu()
    g, c, t = [], [], []
    picked = [r for r in out if r[0][0]][::8]
    for (k, lo, hi, e0, e1, s0, s1), lg in picked:
        win = xc[:, s0:s1]
        g.append(lg.cpu().numpy())
        with torch.no_grad():
            c.append(cls(front(win.unsqueeze(1)).transpose(1, 2).contiguous())[0].numpy()[:, e0 - lo:e1 - lo])
        t.append(ps.truth_logits(csd, ps.truth_sincnet(front, win), 60)[:, e0 - lo:e1 - lo])
    g, c, t = (np.concatenate(a, axis=1) for a in (g, c, t))
    sg, sc = ps.error_stats(g, t), ps.error_stats(c, t)
    print(f"{len(picked)} steps: " + ps.fmt("GPU vs f64 truth", sg))
    print(f"{len(picked)} steps: " + ps.fmt("CPU fp32 vs f64 truth", sc))
    assert any(r[0][2] < W for r in picked) and any(r[0][2] > W for r in picked)
    assert sg["rms"] <= REL * sc["rms"] and sg["max"] <= REL * sc["max"], (sg, sc)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. graph replay

@pytest.mark.parametrize("chunk", [160, 320, 1600])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_graph_replay_equals_eager_and_settles_into_two_graphs(dtype, chunk):
    B, W, L = 5, 48, 7
    m, rt = _model()
    i16 = dtype == torch.int16
    x = _pcm(B, 40000 // chunk * chunk, seed=405 + i16, i16=i16)
    eager, _ = _run(rt, x, chunk, W, L)
    replay, st = _run(rt, x, chunk, W, L, graphs=True)
    bad = [i for i, ((_, a), (_, b)) in enumerate(zip(eager, replay)) if not torch.equal(a, b)]
    print(f"{str(dtype)[6:]} chunk {chunk}: {len(st['graphs'])} graphs for {len(replay)} steps, differing steps {bad[:10]}")
    assert not bad
    assert 1 <= len(st["graphs"]) <= 2
    if chunk == 320:
        assert len(st["graphs"]) == 2
    assert rt.time_chunks() == 1


@pytest.mark.parametrize("mode", ["f16p", "f32"])
def test_graph_replay_on_an_idle_gpu_equals_eager_step_by_step(mode):
    """A device synchronise before every step: each replayed graph starts on an idle GPU."""
    B, W, L, chunk = 5, 48, 7, 320
    m, rt = _model()
    rt.set_gemm_mode(mode)
    x = _pcm(B, 120 * chunk, seed=407, i16=True)
    eager, _ = _run(rt, x, chunk, W, L)
    replay, st = _run(rt, x, chunk, W, L, graphs=True, sync=True)
    bad = [i for i, ((_, a), (_, b)) in enumerate(zip(eager, replay)) if not torch.equal(a, b)]
    print(f"{mode}: {len(st['graphs'])} graphs, {len(replay)} steps, steps differing from eager: {bad[:10]}")
    assert len(st["graphs"]) == 2 and not bad


def test_graphs_are_dropped_after_a_weight_hot_swap():
    from uvad_amd.synth import seed_weights
    B, W, L, chunk = 3, 48, 7, 320
    m, rt = _model()
    x = _pcm(B, 100 * chunk, seed=409, i16=False)
    st = rt.wav_window_stream_open(B, chunk, window=W, lookahead=L, graphs=True)
    for i in range(60):
        rt.wav_window_stream_step(st, x[:, i * chunk:(i + 1) * chunk].contiguous())
    assert st["graphs"]
    seed_weights(m, 999, 4.0)
    rt2 = m.runtime(DEV)
    assert rt2 is rt
    lg = rt.wav_window_stream_step(st, x[:, 60 * chunk:61 * chunk].contiguous()).clone()
    assert len(st["graphs"]) == 1          # the old ones dropped, this step's captured anew
    row = st["frames"]
    J, R = rt.wav_window_geometry()
    lo = row - W
    rt.set_time_chunks(1)
    ref, _ = rt.forward_wav(x[:, J * lo:J * lo + R + J * (W - 1)].contiguous())
    assert torch.equal(lg, ref[:, W - L - lg.shape[1]:W - L])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. refusals

def test_wav_window_refusals():
    import uvad_amd
    from uvad_amd import _lib
    from uvad_amd.runtime import VadRuntime
    m, rt = _model()
    lib, ctx = rt.lib, rt.ctx
    B, chunk, W, L = 4, 320, 40, 7
    st = rt.wav_window_stream_open(B, chunk, window=W, lookahead=L)
    state, ws = st["state"], st["ws"]
    x = torch.zeros((B, 1620), device=DEV)
    xq = torch.zeros((B, chunk), dtype=torch.int16, device=DEV)
    out = torch.empty((B, 8), device=DEV)
    s = rt._stream()

    def step(state_ptr, ld=8, ws_bytes=None, chunk_=chunk, i16=False):
        fn = lib.uvad_window_wav_step_i16 if i16 else lib.uvad_window_wav_step
        return fn(ctx, (xq if i16 else x).data_ptr(), B, chunk_, state_ptr, out.data_ptr(), None, ld, ws.data_ptr(),
                  ws.numel() if ws_bytes is None else ws_bytes, s)

    def err(code, want, text, c=ctx, l=lib):
        assert code == want, (code, l.uvad_last_error(c))
        assert text in l.uvad_last_error(c).decode(), l.uvad_last_error(c)

    err(lib.uvad_window_wav_reset(ctx, state.data_ptr(), B, 0, 0, 0, s), -1, "window must be >= 1")        # W < 1
    err(lib.uvad_window_wav_reset(ctx, state.data_ptr(), B, W, W, 0, s), -1, "lookahead < window")         # L >= W
    assert lib.uvad_window_wav_reset(ctx, state.data_ptr(), B, W, 35, 0, s) == 0
    err(step(state.data_ptr(), chunk_=1620), -1, "exceeds the window")                                      # 35 + ceil(1620 / 270) > 40
    assert lib.uvad_window_wav_reset(ctx, state.data_ptr(), B, W, L, 0, s) == 0
    other = torch.empty_like(state)
    err(step(other.data_ptr()), -3, "uvad_window_wav_reset")                                                # never reset
    err(step(state.data_ptr(), ws_bytes=ws.numel() - 1), -4, "workspace too small")                        # one byte short
    err(step(state.data_ptr(), i16=True), -1, "reset for f32 samples")                                      # wrong sample type
    # ld_out smaller than the k of this step: nothing is enqueued or counted, the next call with room succeeds
    k0, key = C.c_int(), C.c_int64()
    while True:
        assert lib.uvad_window_wav_peek(ctx, state.data_ptr(), chunk, C.byref(k0), C.byref(key)) == 0
        if k0.value:
            break
        assert step(state.data_ptr()) == 0
    err(step(state.data_ptr(), ld=k0.value - 1), -1, "ld_out")
    k1 = C.c_int()
    assert lib.uvad_window_wav_peek(ctx, state.data_ptr(), chunk, C.byref(k1), C.byref(key)) == 0 and k1.value == k0.value
    assert step(state.data_ptr()) == k0.value
    torch.cuda.synchronize()
    # an int16 state refuses the f32 step
    assert lib.uvad_window_wav_reset(ctx, state.data_ptr(), B, W, L, 1, s) == 0
    err(step(state.data_ptr()), -1, "reset for int16 samples")
    assert step(state.data_ptr(), i16=True) == 0
    torch.cuda.synchronize()
    # contexts without SincNet: fbank + model, and fbank only
    lstm = {"hidden_size": 128, "num_layers": 2, "bidirectional": True}
    lin = {"hidden_size": 128, "num_layers": 2}
    fb = VadRuntime(DEV, uvad_amd.FbankConfig(num_filters=64), {"encoding_dim": 64, "lstm": lstm, "linear": lin})
    err(fb.lib.uvad_window_wav_reset(fb.ctx, state.data_ptr(), B, W, L, 0, s), -3, "SincNet", fb.ctx, fb.lib)
    assert fb.lib.uvad_window_wav_state_bytes(fb.ctx, B, W, 0) == 0 and fb.lib.uvad_window_wav_workspace_bytes(fb.ctx, B, chunk, W) == 0
    err(fb.lib.uvad_window_wav_step(fb.ctx, x.data_ptr(), B, chunk, state.data_ptr(), out.data_ptr(), None, 8, ws.data_ptr(), ws.numel(), s),
        -3, "SincNet", fb.ctx, fb.lib)
    with pytest.raises(RuntimeError, match="without a SincNet"):
        fb.wav_window_stream_open(B, chunk)
    only = VadRuntime(DEV, uvad_amd.FbankConfig(num_filters=64))
    err(only.lib.uvad_window_wav_reset(only.ctx, state.data_ptr(), B, W, L, 0, s), -3, "SincNet", only.ctx, only.lib)
    fb.close()
    only.close()
    # the log-mel window stream still refuses a SincNet-only context, as before
    err(lib.uvad_window_reset(ctx, state.data_ptr(), B, W, L, s), -3, "fbank")
    with pytest.raises(RuntimeError, match="FbankConfig"):
        rt.window_stream_open(B, chunk)
    with pytest.raises(_lib.UvadError, match="lookahead < window"):
        rt._check(lib.uvad_window_wav_reset(ctx, state.data_ptr(), B, W, W, 0, s))
    with pytest.raises(ValueError, match="lookahead < window"):
        rt.wav_window_stream_open(B, chunk, window=W, lookahead=W)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the named size

def test_named_size_512_feeds_20ms_chunks_window_293_lookahead_30():
    """512 int16 feeds x 320-sample chunks x ~7 s (past the 5 s warm-up), W = 293, L = 30, the reference PyanNet geometry: every emitted
    frame of every feed is the bits of uvad_forward_wav_i16 on its offline window, and 5 feeds end to end against the float64 truth."""
    from oracle import parity_stats as ps
    from uvad_amd.synth import synth_pcm_device
    torch.set_num_threads(min(16, torch.get_num_threads()))
    front, cls, csd, m = _pair(scale=2.0)
    rt = m.runtime(DEV)
    rt.set_time_chunks(1)
    B, chunk, W, L, S = 512, 320, 293, 30, 16000 * 7
    x = torch.round(synth_pcm_device(B, S, seed=411, device=DEV) * 32767.0).to(torch.int16)
    sub = [0, 1, 255, 256, 511]
    rows, n, bad = [], 0, 0

    def tap(st, row, lg):
        nonlocal n, bad
        k, lo, hi, e0, e1, s0, s1 = row
        if not k:
            return
        ref, _ = rt.forward_wav(x[:, s0:s1].contiguous())
        bad += int(not torch.equal(lg, ref[:, e0 - lo:e1 - lo]))
        n += k
        rows.append((row, lg[sub].cpu().numpy()))

    out, st = _run(rt, x, chunk, W, L, tap=tap)
    warm = [r for r in rows if r[0][2] < W]
    steady = [r for r in rows if r[0][2] > W]
    picked = [warm[len(warm) // 3], warm[-1], steady[len(steady) // 2], steady[-1]]
    last = out[-1][0]
    print(f"named size: {len(out)} steps, {n} frames per feed, steps not bit-identical: {bad}")
    assert last[2] - last[1] == W and n == last[4] and bad == 0
    assert {r[0] for r, _ in out if r[2] > W} == {1, 2}
    assert torch.isfinite(out[-1][1]).all() and rt.time_chunks() == 1
    xs = x[sub].cpu().float() / 32768.0
    worst = 0.0
    for (k, lo, hi, e0, e1, s0, s1), lg in picked:
        t = ps.truth_logits(csd, ps.truth_sincnet(front, xs[:, s0:s1]), 60)[:, e0 - lo:e1 - lo]
        worst = max(worst, float(np.abs(lg - t).max()))
    print(f"named size: 5 feeds x {len(picked)} steps vs the float64 truth {worst:.2e}")
    assert picked and worst < 1e-4
