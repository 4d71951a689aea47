"""GPU tests (-m gpu) of variable-length batches for the SincNet PyanNet (uvad_sincnet_lens[_i16], uvad_forward_wav_lens[_i16]).

Row b of a (B, S) waveform batch holds S_b samples.  Its features (and logits) at t < T_b = uvad_sincnet_num_frames(S_b) must be the
dense call's on wav[b, :S_b] alone -- the waveform norm and the three instance norms over the row's own samples / positions -- and
exactly +0 after.  Lengths sit at the tile edges of both forms of the conv stages (64 pooled outputs per split-f16 tile; pt = 85 / 42 / 42
for the exact form at the reference geometry), at the receptive field R = 991 and at 0.  Checked bit for bit in both forms, from f32 and
int16; the forward bit for bit in modes f32 / f16p_stream with the recurrent tile pinned and to 1e-4 in the launch-size dependent
modes; padding (NaN, 1e30, +-32767) and a workspace of 0xFF bytes change no bit; graph replay with new lengths equals eager enqueue;
the pipeline and predict_vad(ragged_batches=True) give what the per-row paths give."""
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
R = 991
LOGIT_TOL = 1e-4


def _model(seed=11, scale=4.0):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    torch.manual_seed(seed)
    m = uvad_amd.PyanNet()
    m.build()
    seed_weights(m, 1234, scale)
    return m.to(DEV).eval()


def _s_for(stage, pooled):
    """The fewest samples whose stage `stage` (0, 1, 2) gives `pooled` pooled outputs at the reference geometry (stride 10, 251 taps,
    then two 5-tap convs, MaxPool1d(3) each); one sample less gives pooled - 1."""
    L = pooled
    for st in range(stage, -1, -1):
        L = 3 * L + 4 if st > 0 else 10 * (3 * L - 1) + 251
    return L


def _edge_lengths():
    out = []
    for stage, p in ((0, 128), (1, 64), (2, 64), (0, 85), (1, 42), (2, 42)):   # split-form tiles of 64, exact-form tiles of pt
        s = _s_for(stage, p)
        out += [s, s - 1]
    return out


S_MAX = 48000
LENGTHS = [S_MAX, 30011] + _edge_lengths() + [R, R - 1, 0]   # unsorted on purpose


def _wav(B, S, seed):
    from uvad_amd.synth import synth_pcm
    return torch.from_numpy(synth_pcm(B, S, seed=seed)).to(DEV)


def _q(B, S, seed):
    from uvad_amd.synth import synth_pcm
    return torch.from_numpy(np.round(synth_pcm(B, S, seed=seed) * 32767.0).astype(np.int16)).to(DEV)


def _is_pos_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _check_rows(rt, out, x, lens, dense, mode):
    """out: a lens call's (B, T, ...) result; dense(x_row) the dense call on one row alone."""
    for b, n in enumerate(lens):
        T_b = rt.sincnet_num_frames(n) if n >= R else 0
        if T_b > 0:
            want = dense(x[b:b + 1, :n].clone())
            assert rt.sincnet_form() == mode, (b, n)
            torch.cuda.synchronize()
            assert want.shape[1] == T_b
            d = (out[b, :T_b] - want[0]).abs().max().item()
            assert torch.equal(out[b, :T_b], want[0]), (mode, b, n, d)
        assert _is_pos_zero(out[b, T_b:]), (mode, b, n)


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("mode", ["f32", "f16p"])
def test_sincnet_lens_rows_are_the_dense_call_of_each_row_alone(mode, i16):
    m = _model()
    rt = m.runtime(DEV)
    rt.set_gemm_mode(mode)
    B = len(LENGTHS)
    x = (_q if i16 else _wav)(B, S_MAX, seed=17)
    feats = rt.sincnet(x, lengths=LENGTHS).clone()
    assert rt.sincnet_form() == mode
    torch.cuda.synchronize()
    assert feats.shape == (B, rt.sincnet_num_frames(S_MAX), 60)
    _check_rows(rt, feats, x, LENGTHS, lambda r: rt.sincnet(r), mode)
    # all lengths equal to S: the dense call's bits
    full = rt.sincnet(x, lengths=[S_MAX] * B).clone()
    dense = rt.sincnet(x)
    torch.cuda.synchronize()
    assert torch.equal(full, dense)
    rt.set_gemm_mode("f16p")


@pytest.mark.parametrize("mode", ["f32", "f16p_stream", "f16p", "f16p3"])
def test_forward_wav_lens_rows_are_the_dense_forward_of_each_row(mode):
    m = _model()
    rt = m.runtime(DEV)
    rt.set_gemm_mode(mode)
    rt.set_recurrent_tile(4)
    lens = [S_MAX, 20001, _s_for(1, 64) - 1, 0, _s_for(0, 85), R, 40960]
    for i16 in (False, True):
        x = (_q if i16 else _wav)(len(lens), S_MAX, seed=23 + i16)
        logits, probs = (t.clone() for t in rt.forward_wav(x, lengths=lens))
        torch.cuda.synchronize()
        for b, n in enumerate(lens):
            T_b = rt.sincnet_num_frames(n) if n >= R else 0
            if T_b:
                wl, wp = rt.forward_wav(x[b:b + 1, :n].clone())
                torch.cuda.synchronize()
                if mode in ("f32", "f16p_stream"):
                    assert torch.equal(logits[b, :T_b], wl[0]) and torch.equal(probs[b, :T_b], wp[0]), (mode, i16, b, n)
                else:
                    assert (logits[b, :T_b] - wl[0]).abs().max().item() <= LOGIT_TOL, (mode, i16, b, n)
            assert _is_pos_zero(logits[b, T_b:]) and _is_pos_zero(probs[b, T_b:]), (mode, i16, b, n)
    rt.set_recurrent_tile(0)
    rt.set_gemm_mode("f16p")


@pytest.mark.parametrize("mode", ["f32", "f16p"])
def test_padding_and_workspace_contents_are_never_read(mode):
    m = _model()
    rt = m.runtime(DEV)
    rt.set_gemm_mode(mode)
    rt.set_recurrent_tile(4)
    lens = [S_MAX, 17731, 6211, 0, R, 40001]
    B = len(lens)
    x = _wav(B, S_MAX, seed=31)
    q = _q(B, S_MAX, seed=31)
    base_f = rt.sincnet(x, lengths=lens).clone()
    base_q = rt.sincnet(q, lengths=lens).clone()
    base_l = rt.forward_wav(x, lengths=lens)[0].clone()
    torch.cuda.synchronize()
    xp, qp = x.clone(), q.clone()
    for b, n in enumerate(lens):
        xp[b, n:] = float("nan") if b % 2 else 1e30
        xp[b, n::3] = -1e30
        qp[b, n:] = 32767 if b % 2 else -32767
    rt._ws.fill_(255)
    f = rt.sincnet(xp, lengths=lens).clone()
    rt._ws.fill_(255)
    g = rt.sincnet(qp, lengths=lens).clone()
    rt._ws.fill_(255)
    lg = rt.forward_wav(xp, lengths=lens)[0]
    torch.cuda.synchronize()
    assert torch.equal(f, base_f) and torch.equal(g, base_q) and torch.equal(lg, base_l)
    rt.set_recurrent_tile(0)
    rt.set_gemm_mode("f16p")


def test_valid_frames_no_further_from_float64_truth_than_the_fp32_cpu_path():
    """Against the float64 evaluation of each row's prefix alone (oracle/parity_stats.truth_sincnet), with the classifier at weights x4:
    the lens call's features, in both forms, are no further from that truth than torch's fp32 CPU SincNet on the same prefix (within a
    factor 2 of it, plus 1e-6)."""
    import uvad_amd
    from oracle import parity_stats as ps
    from oracle import torch_ref as tr
    front = tr.TorchSincNet().eval()
    csd = tr.seeded_state_dict(60, 128, 4, True, 128, 2, seed=4321, scale=4.0)
    model = {"encoding_dim": 60, "lstm": {"hidden_size": 128, "num_layers": 4, "bidirectional": True},
             "linear": {"hidden_size": 128, "num_layers": 2}, "leaky_slope": 0.01}
    rt = uvad_amd.VadRuntime(DEV, model=model, sincnet=front.config())
    rt.load_state_dict(tr.sincnet_runtime_state_dict(front, csd))
    lens = [24000, 6211, 2791, 16001]
    wav = _wav(len(lens), 24000, seed=41).cpu()
    for mode in ("f32", "f16p"):
        rt.set_gemm_mode(mode)
        got = rt.sincnet(wav.to(DEV), lengths=lens).cpu()
        for b, n in enumerate(lens):
            row = wav[b:b + 1, :n]
            truth = ps.truth_sincnet(front, row).numpy()[0]
            with torch.no_grad():
                cpu = front(row.unsqueeze(1)).transpose(1, 2)[0].numpy()
            T_b = truth.shape[0]
            e_gpu = float(np.abs(got[b, :T_b].numpy().astype(np.float64) - truth).max())
            e_cpu = float(np.abs(cpu.astype(np.float64) - truth).max())
            print(f"{mode} S_b={n}: lens {e_gpu:.2e}, fp32 CPU {e_cpu:.2e}")
            assert e_gpu <= 2.0 * e_cpu + 1e-6, (mode, n, e_gpu, e_cpu)
    rt.set_gemm_mode("f16p")


def test_graph_replay_with_lengths_changed_in_place():
    m = _model()
    rt = m.runtime(DEV)
    rt.set_gemm_mode("f16p_stream")
    rt.set_recurrent_tile(4)
    B, S = 5, 32000
    x = _q(B, S, seed=51)
    lens = torch.tensor([32000, 9000, R, 0, 20000], dtype=torch.int64, device=DEV)
    rt.forward_wav(x, lengths=lens)                       # warm-up: workspace, attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _ = rt.forward_wav(x, lengths=lens)
    for new in ([32000] * 5, [3, 31999, 16000, R - 1, 12345], [0] * 5, [40000, -7, 6211, 6210, 2000]):
        lens.copy_(torch.tensor(new, dtype=torch.int64))
        g.replay()
        torch.cuda.synchronize()
        want, _ = rt.forward_wav(x, lengths=[min(max(v, 0), S) for v in new])
        torch.cuda.synchronize()
        assert torch.equal(out, want), new
    rt.set_recurrent_tile(0)
    rt.set_gemm_mode("f16p")


def test_pipeline_submit_with_lengths_equals_the_runtime_call():
    from uvad_amd.pipeline import ForwardPipeline
    m = _model()
    rt = m.runtime(DEV)
    B, S = 4, 40000
    x = _q(B, S, seed=61)
    lens = [40000, 12000, 0, 25001]
    want_l, want_p = (t.clone() for t in rt.forward_wav(x, lengths=lens))
    torch.cuda.synchronize()
    pipe = ForwardPipeline(m, DEV, 2)
    try:
        got_l, got_p = pipe.submit(x, want_logits=True, want_probs=True, lengths=lens).result()
        torch.cuda.synchronize()
        assert torch.equal(got_l, want_l) and torch.equal(got_p, want_p)
    finally:
        pipe.close()
    # the module tree: forward_ragged; forward / forward_logits keep the reference's signature and point at it
    gl, gp = m.forward_ragged(x.unsqueeze(1), lens)
    assert torch.equal(gl, want_l) and torch.equal(gp, want_p)
    with pytest.raises(NotImplementedError, match="forward_ragged"):
        m.forward_logits(x, lengths=lens)


def _write_wav(path, q):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(q.astype("<i2").tobytes())


def test_predict_vad_ragged_sincnet_gives_the_predictions_of_the_per_length_path(tmp_path, monkeypatch):
    from config.config import load_config
    from src.scripts import predict_vad
    from uvad_amd.synth import synth_pcm
    monkeypatch.setenv("UVAD_FEATURE_EXTRACTOR", "sincnet")
    nsamp = [5 * 16000, 40 * 16000 + 3, 197921, 23 * 16000 + 511, 7 * 16000 + 1, 31 * 16000 + 997]
    paths = []
    for k, n in enumerate(nsamp):
        p = tmp_path / f"w{k}.wav"
        _write_wav(p, np.round(synth_pcm(1, n, seed=800 + k)[0] * 32767.0).astype(np.int16))
        paths.append(str(p))
    cfg = load_config()
    assert cfg.feature_extractor == "sincnet"
    cfg.window_seconds = None
    cfg.max_duration = 90
    cfg.input.kind = "wav"
    cfg.input.paths = paths
    want = predict_vad(**cfg)
    cfg.ragged_batches = True
    got = predict_vad(**cfg)
    assert [r["recording_id"] for r in got] == [r["recording_id"] for r in want]
    for g, w in zip(got, want):
        assert g["num_frames"] == w["num_frames"] > 0
        assert np.array_equal(g["labels"], w["labels"]) and g["intervals"] == w["intervals"]
        assert np.array_equal(g["probs"].view(np.int32), w["probs"].view(np.int32)), g["recording_id"]


def test_refusals_give_their_code_and_message():
    from uvad_amd.runtime import VadRuntime
    m = _model()
    rt = m.runtime(DEV)
    lib, ctx = rt.lib, rt.ctx
    B, S = 2, 16000
    x = _wav(B, S, seed=71)
    n64 = torch.tensor([16000, 5000], dtype=torch.int64, device=DEV)
    T = rt.sincnet_num_frames(S)
    ws = rt._wav_ws(B, S, T, True)
    feats = torch.empty((B, T, 60), device=DEV)
    out = torch.empty((B, T), device=DEV)
    assert lib.uvad_sincnet_lens(ctx, x.data_ptr(), B, S, None, feats.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert b"d_nsamp is NULL" in lib.uvad_last_error(ctx)
    assert lib.uvad_sincnet_lens_i16(ctx, x.data_ptr(), B, S, None, feats.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert b"d_nsamp is NULL" in lib.uvad_last_error(ctx)
    assert lib.uvad_forward_wav_lens(ctx, x.data_ptr(), B, S, None, out.data_ptr(), None, ws.data_ptr(), ws.numel(), None) == -1
    assert b"d_nsamp is NULL" in lib.uvad_last_error(ctx)
    assert lib.uvad_forward_wav_lens_i16(ctx, x.data_ptr(), B, S, None, out.data_ptr(), None, ws.data_ptr(), ws.numel(), None) == -1
    assert b"d_nsamp is NULL" in lib.uvad_last_error(ctx)
    tiny = torch.empty(16, dtype=torch.uint8, device=DEV)
    assert lib.uvad_sincnet_lens(ctx, x.data_ptr(), B, S, n64.data_ptr(), feats.data_ptr(), tiny.data_ptr(), 16, None) == -4
    assert b"workspace too small" in lib.uvad_last_error(ctx)
    assert lib.uvad_forward_wav_lens(ctx, x.data_ptr(), B, S, n64.data_ptr(), out.data_ptr(), None, tiny.data_ptr(), 16, None) == -4
    assert b"workspace too small" in lib.uvad_last_error(ctx)
    # the padded S itself gives no frame: refused as the dense call
    assert lib.uvad_sincnet_lens(ctx, x.data_ptr(), B, R - 1, n64.data_ptr(), feats.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert b"too short" in lib.uvad_last_error(ctx)
    # no SincNet configuration: UVAD_E_STATE
    bare = VadRuntime(DEV, model={"encoding_dim": 60, "lstm": {"hidden_size": 128, "num_layers": 1, "bidirectional": True},
                                  "linear": {"hidden_size": 128, "num_layers": 2}, "leaky_slope": 0.01})
    assert bare.lib.uvad_sincnet_lens(bare.ctx, x.data_ptr(), B, S, n64.data_ptr(), feats.data_ptr(), ws.data_ptr(), ws.numel(),
                                      None) == -3
    assert b"uvad_sincnet_configure" in bare.lib.uvad_last_error(bare.ctx)
    assert bare.lib.uvad_forward_wav_lens(bare.ctx, x.data_ptr(), B, S, n64.data_ptr(), out.data_ptr(), None, ws.data_ptr(),
                                          ws.numel(), None) == -3
    assert b"uvad_sincnet_configure" in bare.lib.uvad_last_error(bare.ctx)
    # host-side validation of list lengths
    with pytest.raises(ValueError, match=r"in \[0, 16000\]"):
        rt.sincnet(x, lengths=[16001, 3])
    with pytest.raises(ValueError, match="2 rows"):
        rt.forward_wav(x, lengths=[5])
