"""GPU tests (-m gpu) of sliding-window inference over whole recordings (uvad_sliding_*; VadRuntime.sliding_classify / sliding_forward /
sliding_forward_wav; predict_vad(hop_seconds=...)).  W = 64 frames and four recordings of 23, 64, 65 and 150 frames: a lone short window,
an exact fit, a second window of W - Hf + 1 frames and a multi-window row with a partial tail.

  tap        every window's probabilities are uvad_classify on that slice of the recording's uvad_fbank_lens features alone (bit for bit
             in GEMM modes f32 / f16p_stream with the recurrent tile pinned; modes f16p / f16p3 to the ragged tests' logit tolerance)
  aggregate  the output against the float64 aggregate of the same f32 tap within 4 (K + 1) 2^-24, K = ceil(W / Hf); hop = window with rect
             weights is the tap laid end to end
  plus group independence, padding never read, a plan one window short, the float64 truth at weights x4, graph replay with new lengths,
  the waveform model, the refusals and predict_vad(hop_seconds=...).
"""
import functools
import wave

import numpy as np
import pytest
import torch

import sliding_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = 64
FRAMES = [23, 64, 65, 150]
LOGIT_TOL = 1e-4                 # tests/test_gpu_ragged.py, modes f16p / f16p3 at weights x2
# the same bound on probabilities: sigmoid is 1/4-Lipschitz, plus one f32 rounding of a value <= 1 on each side
PROB_TOL = LOGIT_TOL / 4 + 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _model(F=64, scale=2.0, window_type="povey"):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet2(encoding_dim=F)
    m.build()
    seed_weights(m, 1234, scale)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type=window_type))
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


@functools.lru_cache(maxsize=None)
def _recordings(seed=7):
    """(pcm (R, S) f32 on the GPU, samples per recording) whose frame counts are FRAMES."""
    from uvad_amd.synth import synth_pcm
    _, rt = _model()
    nsamp = [t * 160 - 37 for t in FRAMES]
    assert [rt.num_frames(n) for n in nsamp] == FRAMES
    S = max(nsamp)
    x = synth_pcm(len(FRAMES), S, seed=seed).copy()
    for r, n in enumerate(nsamp):
        x[r, n:] = 0.0
    return torch.from_numpy(x).to(DEV), nsamp


def _set(rt, mode, tile=4):
    rt.set_gemm_mode(mode)
    rt.set_recurrent_tile(tile)
    rt.set_time_chunks(1)


def _reset(rt):
    rt.set_gemm_mode("f16p")
    rt.set_recurrent_tile(0)
    rt.set_time_chunks(0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _is_pos_zero(t):
    return bool((_bits(t) == 0).all())


def _weights(kind):
    from uvad_amd.postprocess import sliding_weights
    return None if kind == "rect" else sliding_weights(kind, W)


def _check_tap(rt, feats, frames, first, Hf, win, exact):
    """Every window of the plan against the dense classify of its slice alone."""
    worst = 0.0
    for r, T in enumerate(frames):
        for j, (start, n) in enumerate(sr.windows(T, W, Hf, first[r + 1] - first[r])):
            row = win[first[r] + j]
            assert _is_pos_zero(row[n:]), (r, j)
            if n == 0:
                continue
            _, want = rt.classify(feats[r:r + 1, start:start + n].contiguous(), want_logits=False)
            d = float((row[:n] - want[0]).abs().max())
            worst = max(worst, d)
            if exact:
                assert torch.equal(row[:n], want[0]), (r, j, start, n, d)
    return worst


# ---- 1. the window tap -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Hf", [64, 16, 24])
@pytest.mark.parametrize("mode", ["f32", "f16p_stream"])
def test_window_tap_is_bit_identical_to_classify_on_each_slice(mode, Hf):
    m, rt = _model()
    _set(rt, mode)
    pcm, nsamp = _recordings()
    feats = rt.fbank(pcm, lengths=nsamp)
    rt.sliding_configure(W, Hf)
    counts, first = sr.plan(FRAMES, W, Hf)
    probs, frames, win = rt.sliding_forward(pcm, nsamp, tap=True)
    assert rt.recurrent_tile() == 4 and rt.time_chunks() == 1
    assert frames.tolist() == FRAMES and win.shape == (first[-1], W) and probs.shape == (len(FRAMES), max(FRAMES))
    _check_tap(rt, feats, FRAMES, first, Hf, win, exact=True)
    # the same windows from caller-supplied features
    probs_c, frames_c, win_c = rt.sliding_classify(feats, FRAMES, tap=True)
    assert torch.equal(win_c, win) and torch.equal(probs_c, probs) and frames_c.tolist() == FRAMES
    _reset(rt)


@pytest.mark.parametrize("mode", ["f16p", "f16p3"])
def test_window_tap_in_launch_size_dependent_modes_agrees_to_the_bound(mode):
    m, rt = _model()
    rt.set_gemm_mode(mode)
    pcm, nsamp = _recordings()
    feats = rt.fbank(pcm, lengths=nsamp)
    worst = 0.0
    for Hf in (64, 16, 24):
        rt.sliding_configure(W, Hf)
        _, first = sr.plan(FRAMES, W, Hf)
        _, _, win = rt.sliding_forward(pcm, nsamp, tap=True)
        worst = max(worst, _check_tap(rt, feats, FRAMES, first, Hf, win, exact=False))
    print(f"{mode}: max |window tap - dense classify| = {worst:.2e} (bound {PROB_TOL:.2e})")
    assert worst <= PROB_TOL
    _reset(rt)


# ---- 2. the aggregate ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rect", "hamming"])
@pytest.mark.parametrize("Hf", [64, 16, 24])
def test_aggregate_against_float64_on_the_same_tap(Hf, kind):
    m, rt = _model()
    _set(rt, "f32")
    pcm, nsamp = _recordings()
    w = _weights(kind)
    rt.sliding_configure(W, Hf, w)
    _, first = sr.plan(FRAMES, W, Hf)
    probs, frames, win = rt.sliding_forward(pcm, nsamp, tap=True)
    got, tap = probs.cpu().numpy(), win.cpu().numpy()
    want = sr.aggregate_f64(tap, FRAMES, first, W, Hf, w, T_out=got.shape[1])
    K = -(-W // Hf)
    bound = 4 * (K + 1) * 2.0 ** -24
    err = float(np.abs(got.astype(np.float64) - want).max())
    same = np.array_equal(got, sr.aggregate_f32(tap, FRAMES, first, W, Hf, w, T_out=got.shape[1]))
    print(f"Hf={Hf} {kind}: max |aggregate - float64| = {err:.2e} (bound {bound:.2e}); equals the f32 ascending-j form: {same}")
    assert err <= bound
    assert same
    for r, T in enumerate(FRAMES):
        assert _is_pos_zero(probs[r, T:])
    if Hf == W and kind == "rect":   # hop = window: the windows laid end to end
        for r, T in enumerate(FRAMES):
            assert torch.equal(probs[r, :T], win[first[r]:first[r + 1]].reshape(-1)[:T])
    _reset(rt)


# ---- 3. group independence -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "f16p_stream"])
def test_result_does_not_depend_on_the_group_size(mode):
    m, rt = _model()
    _set(rt, mode)
    pcm, nsamp = _recordings()
    Hf = 16
    rt.sliding_configure(W, Hf, _weights("hamming"))
    N = sr.plan(FRAMES, W, Hf)[1][-1]
    assert N == 11
    ref = None
    for group in (1, 3, N):
        probs, frames, win = rt.sliding_forward(pcm, nsamp, group=group, tap=True)
        got = (probs.clone(), win.clone(), frames.clone())
        if ref is None:
            ref = got
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ref[:2], got[:2])) and torch.equal(ref[2], got[2]), group
    _reset(rt)


# ---- 4. padding ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", [float("nan"), float("inf"), 1e30])
def test_padding_is_never_read(poison):
    m, rt = _model()
    _set(rt, "f16p_stream")
    pcm, nsamp = _recordings()
    Hf = 24
    rt.sliding_configure(W, Hf, _weights("hamming"))
    feats = rt.fbank(pcm, lengths=nsamp)
    clean_f = tuple(t.clone() for t in rt.sliding_forward(pcm, nsamp, tap=True))
    clean_c = tuple(t.clone() for t in rt.sliding_classify(feats, FRAMES, tap=True))
    bad_pcm, bad_feats = pcm.clone(), feats.clone()
    for r, (n, T) in enumerate(zip(nsamp, FRAMES)):
        bad_pcm[r, n:] = poison
        bad_feats[r, T:] = poison
    got_f = rt.sliding_forward(bad_pcm, nsamp, tap=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(clean_f, got_f))
    got_c = rt.sliding_classify(bad_feats, FRAMES, tap=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(clean_c, got_c))
    for probs, frames, _ in (got_f, got_c):
        assert frames.tolist() == FRAMES
        for r, T in enumerate(FRAMES):
            assert _is_pos_zero(probs[r, T:]) and bool(torch.isfinite(probs[r, :T]).all())
    _reset(rt)


# ---- 5. a short plan -------------------------------------------------------------------------------------------------------------------

def test_a_plan_one_window_short_gives_zero_on_the_uncovered_frames():
    m, rt = _model()
    _set(rt, "f32")
    pcm, nsamp = _recordings()
    Hf = 16
    rt.sliding_configure(W, Hf)
    counts, first = sr.plan(FRAMES, W, Hf)
    full, _, win = rt.sliding_forward(pcm, nsamp, tap=True)
    full, win = full.clone(), win.clone()
    short = list(first)
    short[-1] -= 1                                             # the last recording (150 frames, 7 windows) gets 6
    probs, frames, win_s = rt.sliding_forward(pcm, nsamp, first=short, tap=True)
    assert frames.tolist() == FRAMES and torch.equal(win_s, win[:-1])
    covered = (counts[-1] - 2) * Hf + W                        # the 6 windows reach frame 144
    lost = (counts[-1] - 1) * Hf                               # the dropped window covered [96, 150)
    assert (covered, lost) == (144, 96)
    assert _is_pos_zero(probs[3, covered:]) and not _is_pos_zero(full[3, covered:FRAMES[3]])
    assert torch.equal(_bits(probs[:3]), _bits(full[:3])) and torch.equal(_bits(probs[3, :lost]), _bits(full[3, :lost]))
    want = sr.aggregate_f32(win_s.cpu().numpy(), FRAMES, short, W, Hf, None, T_out=probs.shape[1])
    assert np.array_equal(probs.cpu().numpy(), want)
    _reset(rt)


# ---- 6. float64 truth ------------------------------------------------------------------------------------------------------------------

def test_aggregate_no_further_from_float64_truth_than_the_cpu_path():
    """Weights x4 (the near-chaotic network): truth = the float64 aggregate of sigmoid(float64 logits) of every window; the fp32 CPU
    path's windows are aggregated the same way."""
    from oracle import parity_stats as ps, torch_ref as tr
    F, Hf = 64, 16
    m, rt = _model(F, 4.0)
    rt.set_gemm_mode("f16p")
    pcm, nsamp = _recordings()
    w = _weights("hamming")
    rt.sliding_configure(W, Hf, w)
    feats = rt.fbank(pcm, lengths=nsamp)
    probs, _ = rt.sliding_classify(feats, FRAMES)
    _, first = sr.plan(FRAMES, W, Hf)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    cpu = tr.TorchPyanNet2(F)
    cpu.load_state_dict(sd)
    fh = feats.cpu()
    win_t, win_c = np.zeros((first[-1], W)), np.zeros((first[-1], W))
    for r, T in enumerate(FRAMES):
        for j, (start, n) in enumerate(sr.windows(T, W, Hf)):
            x = fh[r:r + 1, start:start + n]
            win_t[first[r] + j, :n] = 1.0 / (1.0 + np.exp(-ps.truth_logits(sd, x, F)[0]))
            with torch.no_grad():
                win_c[first[r] + j, :n] = torch.sigmoid(cpu(x)[0])[0].numpy()
    truth = sr.aggregate_f64(win_t, FRAMES, first, W, Hf, w)
    cpu_agg = sr.aggregate_f64(win_c, FRAMES, first, W, Hf, w)
    valid = np.concatenate([np.arange(T) + r * max(FRAMES) for r, T in enumerate(FRAMES)])
    g = probs.cpu().numpy().astype(np.float64).ravel()[valid]
    sg, sc = ps.error_stats(g, truth.ravel()[valid]), ps.error_stats(cpu_agg.ravel()[valid], truth.ravel()[valid])
    print(ps.fmt("GPU sliding vs f64 truth", sg))
    print(ps.fmt("CPU fp32 vs f64 truth", sc))
    assert sg["rms"] <= 1.5 * sc["rms"], (sg, sc)
    _reset(rt)


# ---- 7. graph capture ------------------------------------------------------------------------------------------------------------------

def test_graph_replay_with_new_lengths_under_the_same_plan():
    m, rt = _model()
    rt.set_gemm_mode("f16p")
    pcm, nsamp = _recordings()
    Hf = 16
    rt.sliding_configure(W, Hf, _weights("hamming"))
    _, first = sr.plan(FRAMES, W, Hf)
    R, S = pcm.shape
    T, N = rt.num_frames(S), first[-1]
    lib, ctx = rt.lib, rt.ctx
    d_n = torch.tensor(nsamp, dtype=torch.int64, device=DEV)
    d_first = torch.tensor(first, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.uvad_sliding_workspace_bytes(ctx, R, T, N, 4)), dtype=torch.uint8, device=DEV)
    out = torch.empty((R, T), device=DEV)
    frames = torch.empty(R, dtype=torch.int32, device=DEV)

    def enqueue():
        rt._check(lib.uvad_sliding_forward(ctx, pcm.data_ptr(), R, S, d_n.data_ptr(), d_first.data_ptr(), N, 4, out.data_ptr(), T,
                                           frames.data_ptr(), None, ws.data_ptr(), ws.numel(), rt._stream()))

    enqueue()                                                  # warm-up: kernel attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    for new in (nsamp, [nsamp[1], nsamp[0], nsamp[3], nsamp[2]], [0, 399, S, 12345], [S + 99, -5, 160 * 70, 160 * 64]):
        d_n.copy_(torch.tensor(new, dtype=torch.int64))
        g.replay()
        torch.cuda.synchronize()
        clamped = [min(max(v, 0), S) for v in new]
        want, want_frames = rt.sliding_forward(pcm, clamped, group=4, first=first)
        assert torch.equal(_bits(out), _bits(want)) and torch.equal(frames, want_frames), new
        assert frames.tolist() == [rt.num_frames(v) for v in clamped]
    _reset(rt)


# ---- 8. the waveform model -------------------------------------------------------------------------------------------------------------

J, R0 = 270, 991
S_W = R0 + J * (W - 1)


@functools.lru_cache(maxsize=None)
def _wav_model():
    import uvad_amd
    from uvad_amd.synth import seed_weights
    torch.manual_seed(11)
    m = uvad_amd.PyanNet()
    m.build()
    seed_weights(m, 1234, 4.0)
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


@functools.lru_cache(maxsize=None)
def _wav_recordings(i16):
    from uvad_amd.synth import synth_pcm
    nsamp = [R0 + J * (t - 1) + 100 for t in FRAMES]
    x = synth_pcm(len(FRAMES), max(nsamp), seed=19).copy()
    for r, n in enumerate(nsamp):
        x[r, n:] = 0.0
    if i16:
        return torch.from_numpy(np.round(x * 32767.0).astype(np.int16)).to(DEV), nsamp
    return torch.from_numpy(x).to(DEV), nsamp


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("mode", ["f32", "f16p_stream"])
def test_waveform_windows_are_forward_wav_on_each_clip_and_aggregate(mode, i16):
    m, rt = _wav_model()
    _set(rt, mode)
    x, nsamp = _wav_recordings(i16)
    assert [rt.sincnet_num_frames(n) for n in nsamp] == FRAMES
    for Hf in (W, W // 4):
        rt.sliding_configure(W, Hf, _weights("hamming"))
        _, first = sr.plan(FRAMES, W, Hf)
        probs, frames, win = rt.sliding_forward_wav(x, nsamp, group=5, tap=True)
        probs, win = probs.clone(), win.clone()
        assert frames.tolist() == FRAMES and rt.time_chunks() == 1
        for r, T in enumerate(FRAMES):
            for j, (start, n) in enumerate(sr.windows(T, W, Hf)):
                clip = min(nsamp[r] - J * start, S_W)
                assert rt.sincnet_num_frames(clip) == n
                _, want = rt.forward_wav(x[r:r + 1, J * start:J * start + clip].clone(), want_logits=False)
                row = win[first[r] + j]
                assert torch.equal(row[:n], want[0]), (mode, i16, Hf, r, j, float((row[:n] - want[0]).abs().max()))
                assert _is_pos_zero(row[n:])
        got, tap = probs.cpu().numpy(), win.cpu().numpy()
        want = sr.aggregate_f64(tap, FRAMES, first, W, Hf, _weights("hamming"), T_out=got.shape[1])
        K = -(-W // Hf)
        err = float(np.abs(got - want).max())
        print(f"wav {mode} i16={i16} Hf={Hf}: max |aggregate - float64| = {err:.2e}")
        assert err <= 4 * (K + 1) * 2.0 ** -24
        for r, T in enumerate(FRAMES):
            assert _is_pos_zero(probs[r, T:])
    _reset(rt)


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), 1e30])
def test_waveform_padding_is_never_read(poison):
    m, rt = _wav_model()
    _set(rt, "f16p_stream")
    x, nsamp = _wav_recordings(False)
    rt.sliding_configure(W, 16)
    clean = tuple(t.clone() for t in rt.sliding_forward_wav(x, nsamp, tap=True))
    bad = x.clone()
    for r, n in enumerate(nsamp):
        bad[r, n:] = poison
    got = rt.sliding_forward_wav(bad, nsamp, tap=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(clean, got))
    assert got[1].tolist() == FRAMES
    for r, T in enumerate(FRAMES):
        assert _is_pos_zero(got[0][r, T:]) and bool(torch.isfinite(got[0][r, :T]).all())
    _reset(rt)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_give_their_code_and_message():
    m, rt = _model()
    lib, ctx = rt.lib, rt.ctx
    pcm, nsamp = _recordings()
    R, S = pcm.shape
    T = rt.num_frames(S)
    feats = rt.fbank(pcm, lengths=nsamp)
    d_n = torch.tensor(nsamp, dtype=torch.int64, device=DEV)
    d_t = torch.tensor(FRAMES, dtype=torch.int32, device=DEV)
    out = torch.empty((R, T), device=DEV)
    frames = torch.empty(R, dtype=torch.int32, device=DEV)

    def err(c=ctx):
        return lib.uvad_last_error(c)

    # configure
    ones = np.ones(W, np.float32)
    for hop in (0, W + 1, -3):
        assert lib.uvad_sliding_configure(ctx, W, hop, None) == -1 and b"1 <= hop <= window" in err()
    assert lib.uvad_sliding_configure(ctx, 0, 1, None) == -1 and b"window must be >= 1" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        w = ones.copy()
        w[5] = bad
        assert lib.uvad_sliding_configure(ctx, W, 16, w.ctypes.data) == -1 and b"finite and > 0 (weight 5)" in err()
    # not configured: a fresh context with the same model
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m2 = uvad_amd.PyanNet2(encoding_dim=64)
    m2.build()
    seed_weights(m2, 1234, 2.0)
    m2.attach_fbank(uvad_amd.FbankConfig(num_filters=64, window_type="povey"))
    fresh = m2.to(DEV).eval().runtime(DEV)
    big = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    d_first = torch.tensor(sr.plan(FRAMES, W, 16)[1], dtype=torch.int32, device=DEV)
    args_f = (pcm.data_ptr(), R, S, d_n.data_ptr(), d_first.data_ptr(), 11, 4, out.data_ptr(), T, frames.data_ptr(), None)
    assert fresh.lib.uvad_sliding_forward(fresh.ctx, *args_f, big.data_ptr(), big.numel(), None) == -3
    assert b"uvad_sliding_configure has not been called" in err(fresh.ctx)
    assert fresh.lib.uvad_sliding_workspace_bytes(fresh.ctx, R, T, 11, 4) == 0
    with pytest.raises(RuntimeError, match="sliding_configure"):
        fresh.sliding_forward(pcm, nsamp)
    # the calls
    rt.sliding_configure(W, 16)
    need = int(lib.uvad_sliding_workspace_bytes(ctx, R, T, 11, 4))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    tail = (ws.data_ptr(), ws.numel(), None)

    def fwd(nsamp_p=d_n.data_ptr(), first_p=d_first.data_ptr(), N=11, group=4, ld=T, wsz=ws.numel()):
        return lib.uvad_sliding_forward(ctx, pcm.data_ptr(), R, S, nsamp_p, first_p, N, group, out.data_ptr(), ld, frames.data_ptr(), None,
                                        ws.data_ptr(), wsz, None)

    assert fwd() == 0
    assert fwd(group=0) == -1 and b"group must be >= 1" in err()
    assert fwd(N=-1) == -1 and b"N must be in" in err()
    assert fwd(first_p=None) == -1 and b"d_first is NULL" in err()
    assert fwd(nsamp_p=None) == -1 and b"lengths are NULL" in err()
    assert fwd(ld=T - 1) == -1 and b"ld_out must be at least" in err()
    assert fwd(wsz=need - 1) == -4 and f"need {need} bytes".encode() in err()
    assert lib.uvad_sliding_forward_i16(ctx, pcm.data_ptr(), R, S, d_n.data_ptr(), d_first.data_ptr(), 11, 0, out.data_ptr(), T,
                                        frames.data_ptr(), None, *tail) == -1 and b"uvad_sliding_forward_i16: group" in err()
    cls = (feats.data_ptr(), R, T)
    assert lib.uvad_sliding_classify(ctx, *cls, d_t.data_ptr(), d_first.data_ptr(), 11, 4, out.data_ptr(), T, frames.data_ptr(), None, *tail) == 0
    assert lib.uvad_sliding_classify(ctx, *cls, None, d_first.data_ptr(), 11, 4, out.data_ptr(), T, frames.data_ptr(), None, *tail) == -1
    assert b"lengths are NULL" in err()
    assert lib.uvad_sliding_classify(ctx, *cls, d_t.data_ptr(), None, 11, 4, out.data_ptr(), T, frames.data_ptr(), None, *tail) == -1
    assert b"d_first is NULL" in err()
    assert lib.uvad_sliding_classify(ctx, *cls, d_t.data_ptr(), d_first.data_ptr(), 11, 4, out.data_ptr(), T, frames.data_ptr(), None,
                                     ws.data_ptr(), 16, None) == -4 and b"workspace too small: need" in err()
    # the waveform entries on a context without a SincNet configuration, and unconfigured / refused on one with it
    assert lib.uvad_sliding_forward_wav(ctx, pcm.data_ptr(), R, S, d_n.data_ptr(), d_first.data_ptr(), 11, 4, out.data_ptr(), T,
                                        frames.data_ptr(), None, *tail) == -3 and b"SincNet configuration" in err()
    assert lib.uvad_sliding_wav_workspace_bytes(ctx, R, S, 11, 4) == 0
    mw, rtw = _wav_model()
    x, ns = _wav_recordings(False)
    rtw.sliding_configure(W, 16)
    Sw = x.shape[1]
    Tw = rtw.sincnet_num_frames(Sw)
    d_nw = torch.tensor(ns, dtype=torch.int64, device=DEV)
    needw = int(rtw.lib.uvad_sliding_wav_workspace_bytes(rtw.ctx, R, Sw, 11, 4))
    wsw = torch.empty(needw, dtype=torch.uint8, device=DEV)
    outw = torch.empty((R, Tw), device=DEV)

    def wav(fn=rtw.lib.uvad_sliding_forward_wav, nsamp_p=d_nw.data_ptr(), first_p=d_first.data_ptr(), N=11, group=4, wsz=needw):
        return fn(rtw.ctx, x.data_ptr(), R, Sw, nsamp_p, first_p, N, group, outw.data_ptr(), Tw, frames.data_ptr(), None, wsw.data_ptr(), wsz, None)

    assert needw > 0 and wav() == 0
    assert wav(group=0) == -1 and b"group must be >= 1" in err(rtw.ctx)
    assert wav(N=-2) == -1 and b"N must be in" in err(rtw.ctx)
    assert wav(first_p=None) == -1 and b"d_first is NULL" in err(rtw.ctx)
    assert wav(nsamp_p=None) == -1 and b"lengths are NULL" in err(rtw.ctx)
    assert wav(wsz=needw - 1) == -4 and f"need {needw} bytes".encode() in err(rtw.ctx)
    assert wav(fn=rtw.lib.uvad_sliding_forward_wav_i16, group=0) == -1 and b"uvad_sliding_forward_wav_i16" in err(rtw.ctx)
    torch.cuda.synchronize()
    # host side
    with pytest.raises(ValueError, match="prefix sums"):
        rt.sliding_forward(pcm, nsamp, first=[0, 1, 2])
    with pytest.raises(ValueError, match="shape"):
        rt.sliding_configure(W, 16, np.ones(W + 1, np.float32))


# ---- 10. predict_vad -------------------------------------------------------------------------------------------------------------------

def _write_wav(path, x):
    q = np.round(x * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(q.tobytes())
    return q


def test_predict_vad_with_hop_seconds(tmp_path):
    from config.config import load_config
    from src.scripts import predict_vad
    from uvad_amd.postprocess import labels_to_intervals, median_window, sliding_weights
    from uvad_amd.synth import synth_pcm
    secs = [6.2, 12.37, 3.0]                                   # 3.0 s: the cuts drop it whole, the sliding path keeps it
    paths, pcm16 = [], []
    for k, s in enumerate(secs):
        p = tmp_path / f"r{k}.wav"
        pcm16.append(_write_wav(p, synth_pcm(1, int(s * 16000), seed=500 + k)[0]))
        paths.append(str(p))
    cfg = load_config()
    cfg.model_dict.encoding_dim = 64
    cfg.weights_scale = 2.0
    cfg.max_duration = 90
    cfg.input.kind = "wav"
    cfg.input.paths = paths
    # hop_seconds=None: today's path, byte for byte what the call without the key gives
    assert cfg.hop_seconds is None
    explicit = predict_vad(**cfg)
    untouched = predict_vad(**{k: v for k, v in cfg.items() if not k.startswith(("hop_", "sliding_"))})
    assert len(explicit) == len(untouched) == 3
    for a, b in zip(explicit, untouched):
        assert a["recording_id"] == b["recording_id"] and a["num_frames"] == b["num_frames"] and a["intervals"] == b["intervals"]
        assert a["labels"].tobytes() == b["labels"].tobytes() and a["probs"].tobytes() == b["probs"].tobytes()
    assert explicit[2]["num_frames"] == 0                      # the 3 s recording: dropped by the cuts
    # hop_seconds = 2.5: windows of 500 frames every 250
    cfg.hop_seconds = 2.5
    got = predict_vad(**cfg)
    m, rt = _model(64, 2.0)
    rt.set_gemm_mode("f16p")
    rt.set_recurrent_tile(0)
    Wf, Hf = rt.num_frames(80000), 250
    assert Wf == 500
    rt.sliding_configure(Wf, Hf, sliding_weights("hamming", Wf))
    order = sorted(range(3), key=lambda i: (-len(pcm16[i]), i))
    x = torch.zeros((3, max(len(q) for q in pcm16)), dtype=torch.int16, device=DEV)
    for r, i in enumerate(order):
        x[r, :len(pcm16[i])] = torch.from_numpy(pcm16[i].astype(np.int16)).to(DEV)
    probs, frames = rt.sliding_forward(x, [len(pcm16[i]) for i in order])
    half = median_window(0.01) // 2
    for r, i in enumerate(order):
        res = got[i]
        T = int(frames[r])
        assert res["recording_id"] == f"r{i}.wav" and res["num_frames"] == T == rt.num_frames(len(pcm16[i])) > 0
        want = probs[r, :T].cpu().numpy()
        assert res["probs"].tobytes() == want.tobytes()
        hard = np.concatenate([np.zeros(half, np.int64), (want >= 0.5).astype(np.int64), np.zeros(half, np.int64)])
        lab = np.array([int(hard[t:t + 2 * half + 1].sum() > half) for t in range(T)], np.uint8)
        assert np.array_equal(res["labels"], lab)
        assert res["intervals"] == labels_to_intervals(lab, cfg.frame_shift)
    _reset(rt)
