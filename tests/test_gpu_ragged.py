"""GPU tests (-m gpu) of variable-length batches (uvad_*_lens; VadRuntime.classify / forward / fbank / median_filter / label_runs with
lengths=...): pack_padded_sequence semantics for a bidirectional PyanNet2.

  identity   every valid frame of a ragged batch is bit for bit the dense uvad_classify of the rows of that length at T = len
             (GEMM modes f32 and f16p_stream, recurrent tile pinned to 4 and 16, time chunks off); modes f16p / f16p3 to LOGIT_TOL
  truth      at weights x4 the valid frames are no further from the float64 truth of each prefix than the fp32 CPU path (1.5 x rms)
  padding    frames past a length are never read (NaN / 1e6 there change no bit) and come out as exactly 0
  plus all-lengths-equal-T against the dense calls, a causal model, the front end, median / runs, graph replay, predict_vad and
  the refusals.
"""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4


def _model(F, H=128, scale=2.0, bidirectional=True, window_type="povey"):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    dev = torch.device("cuda:0")
    m = uvad_amd.PyanNet2(lstm={"bidirectional": bidirectional, "hidden_size": H}, encoding_dim=F)
    m.build()
    seed_weights(m, 1234, scale)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type=window_type))
    m = m.to(dev).eval()
    return m, m.runtime(dev)


def _feats(rt, B, T, seed):
    """Realistic log-mel features (B, T, F) from synthetic speech."""
    from uvad_amd.synth import synth_pcm
    S = T * 160
    return rt.fbank(torch.from_numpy(synth_pcm(B, S, seed=seed)).cuda())[:, :T].contiguous()


def _dense_per_length(rt, feats, lens):
    """{row: logits (len,)} from dense uvad_classify on the rows of each length at T = len."""
    out = {}
    for L in sorted(set(lens)):
        if L == 0:
            continue
        idx = [b for b, n in enumerate(lens) if n == L]
        lg, _ = rt.classify(feats[idx, :L].contiguous())
        for k, b in enumerate(idx):
            out[b] = lg[k]
    return out


LENS_7 = [37, 1, 90, 0, 64, 89, 17]          # unsorted, with 1, T and 0; B = 7 (not a multiple of 4 or 16)


@pytest.mark.parametrize("F,H,tile", [(64, 128, 4), (64, 128, 16), (80, 128, 4), (80, 128, 16), (64, 64, 4), (80, 96, 4)])
@pytest.mark.parametrize("mode", ["f32", "f16p_stream"])
def test_valid_frames_are_bit_identical_to_dense_classify_of_each_length(F, H, tile, mode):
    T = 90
    m, rt = _model(F, H)
    rt.set_gemm_mode(mode)
    rt.set_recurrent_tile(tile)
    rt.set_time_chunks(1)
    lens = LENS_7 if tile == 4 else LENS_7 + [90, 3, 55, 12, 90, 71, 8, 44, 66, 29, 90]   # 18 rows: two 16-sequence workgroups
    B = len(lens)
    feats = _feats(rt, B, T, seed=11 + F + H)
    lg, pr = rt.classify(feats, lengths=lens)
    assert rt.recurrent_tile() == tile and rt.time_chunks() == 1
    want = _dense_per_length(rt, feats, lens)
    for b, L in enumerate(lens):
        if L:
            assert torch.equal(lg[b, :L], want[b]), (b, L, float((lg[b, :L] - want[b]).abs().max()))
        assert torch.count_nonzero(lg[b, L:]) == 0 and torch.count_nonzero(pr[b, L:]) == 0
        assert torch.equal(pr[b, :L], torch.sigmoid(lg[b, :L])) or float((pr[b, :L] - torch.sigmoid(lg[b, :L])).abs().max()) < 1e-6


@pytest.mark.parametrize("mode", ["f16p", "f16p3"])
def test_modes_with_launch_size_dependent_kernels_agree_with_dense_to_the_bound(mode):
    """Modes f16p / f16p3 pick the weight-stationary projection, the fused head and the recurrent form by launch size, so a ragged
    batch and a dense call of fewer rows may run different (equivalent) kernels: agreement to LOGIT_TOL at weights x2.  Whether the bits
    also agree is reported, not asserted."""
    T, F = 300, 64
    m, rt = _model(F)
    rt.set_gemm_mode(mode)
    lens = [300, 1, 157, 0, 299, 64, 300, 211, 5, 90, 180]
    feats = _feats(rt, len(lens), T, seed=21)
    lg, _ = rt.classify(feats, lengths=lens)
    want = _dense_per_length(rt, feats, lens)
    worst, same = 0.0, True
    for b, L in enumerate(lens):
        if L:
            worst = max(worst, float((lg[b, :L] - want[b]).abs().max()))
            same &= bool(torch.equal(lg[b, :L], want[b]))
        assert torch.count_nonzero(lg[b, L:]) == 0
    print(f"{mode}: max |ragged - dense| = {worst:.2e}, bit-identical: {same}")
    assert worst < LOGIT_TOL


def test_valid_frames_no_further_from_float64_truth_than_the_cpu_path():
    """Weights x4 (the near-chaotic network): every row's valid frames against the float64 truth of its prefix alone."""
    from oracle import parity_stats as ps, torch_ref as tr
    F, T = 64, 200
    m, rt = _model(F, scale=4.0)
    lens = [200, 13, 150, 77, 1, 199]
    feats = _feats(rt, len(lens), T, seed=31)
    lg, _ = rt.classify(feats, lengths=lens)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    cpu = tr.TorchPyanNet2(F)
    cpu.load_state_dict(sd)
    fh = feats.cpu()
    g, c, t = [], [], []
    for b, L in enumerate(lens):
        g.append(lg[b, :L].cpu().numpy())
        with torch.no_grad():
            c.append(cpu(fh[b:b + 1, :L])[0].numpy()[0])
        t.append(ps.truth_logits(sd, fh[b:b + 1, :L], F)[0])
    g, c, t = (np.concatenate(a) for a in (g, c, t))
    sg, sc = ps.error_stats(g, t), ps.error_stats(c, t)
    print(ps.fmt("GPU ragged vs f64 truth", sg))
    print(ps.fmt("CPU fp32 vs f64 truth", sc))
    assert sg["rms"] <= 1.5 * sc["rms"], (sg, sc)


@pytest.mark.parametrize("mode", ["f32", "f16p", "f16p_stream", "f16p3"])
def test_all_lengths_equal_T_is_bit_identical_to_the_dense_calls(mode):
    from uvad_amd.synth import synth_pcm
    F, B, S = 64, 6, 16000 * 3 + 37
    m, rt = _model(F)
    rt.set_gemm_mode(mode)
    x = torch.from_numpy(synth_pcm(B, S, seed=41)).cuda()
    T = rt.num_frames(S)
    feats = rt.fbank(x)
    d_lg, d_pr = rt.classify(feats)
    r_lg, r_pr = rt.classify(feats, lengths=torch.full((B,), T, dtype=torch.int32, device="cuda"))
    assert torch.equal(d_lg, r_lg) and torch.equal(d_pr, r_pr)
    d_lg, d_pr = rt.forward(x)
    r_lg, r_pr = rt.forward(x, lengths=[S] * B)
    assert torch.equal(d_lg, r_lg) and torch.equal(d_pr, r_pr)
    xi = (x * 32767).round().to(torch.int16)
    assert torch.equal(rt.forward(xi)[0], rt.forward(xi, lengths=[S] * B)[0])


def test_causal_model_valid_frames_equal_the_dense_call_at_the_same_shape():
    F, T = 64, 120
    m, rt = _model(F, bidirectional=False)
    lens = [120, 5, 0, 77, 119]
    feats = _feats(rt, len(lens), T, seed=51)
    d_lg, _ = rt.classify(feats)
    r_lg, _ = rt.classify(feats, lengths=lens)
    for b, L in enumerate(lens):
        assert torch.equal(r_lg[b, :L], d_lg[b, :L])
        assert torch.count_nonzero(r_lg[b, L:]) == 0


@pytest.mark.parametrize("mode", ["f32", "f16p"])
def test_padding_is_never_read(mode):
    """NaN in the padding frames / samples changes no valid bit; in the split-f16 mode a 1e6 in the padding (outside the f16 range)
    gives the bits of clean padding, i.e. the range check never sees it; padding outputs are exactly 0."""
    from uvad_amd.synth import synth_pcm
    F, T = 64, 100
    m, rt = _model(F)
    rt.set_gemm_mode(mode)
    lens = [100, 40, 1, 0, 73]
    feats = _feats(rt, len(lens), T, seed=61)
    clean = feats.clone()
    nan, big = feats.clone(), feats.clone()
    for b, L in enumerate(lens):
        clean[b, L:] = 0.0
        nan[b, L:] = float("nan")
        big[b, L:] = 1e6
    want_lg, want_pr = rt.classify(clean, lengths=lens)
    for poisoned in (nan, big):
        lg, pr = rt.classify(poisoned, lengths=lens)
        assert torch.equal(lg, want_lg) and torch.equal(pr, want_pr)
    for b, L in enumerate(lens):
        assert torch.all(want_lg[b, L:] == 0) and torch.all(want_pr[b, L:] == 0)
        assert not torch.signbit(want_lg[b, L:]).any()
    # PCM: NaN past S_b
    S = 16000 * 2
    nsamp = [S, 16000, 12345, 0, 400]
    x = torch.from_numpy(synth_pcm(len(nsamp), S, seed=62)).cuda()
    xn = x.clone()
    for b, n in enumerate(nsamp):
        x[b, n:] = 0.0
        xn[b, n:] = float("nan")
    lg0, pr0 = rt.forward(x, lengths=nsamp)
    lg1, pr1 = rt.forward(xn, lengths=nsamp)
    assert torch.equal(lg0, lg1) and torch.equal(pr0, pr1)
    assert torch.isfinite(lg0).all()
    for b, n in enumerate(nsamp):
        Tb = rt.num_frames(n)
        assert torch.count_nonzero(lg0[b, Tb:]) == 0


@pytest.mark.parametrize("i16", [False, True])
def test_fbank_lens_matches_fbank_of_each_row_alone(i16):
    from uvad_amd.synth import synth_pcm
    F = 80
    m, rt = _model(F)
    S = 160 * 300 + 7
    nsamp = [160 * 200, 160 * 150 + 79, 160 * 37 + 80, 160 * 299 + 159, S, 79, 0, 160 * 2 + 80]
    x = torch.from_numpy(synth_pcm(len(nsamp), S, seed=71)).cuda()
    if i16:
        x = (x * 32767).round().to(torch.int16)
    got = rt.fbank(x, lengths=nsamp)
    T = rt.num_frames(S)
    assert got.shape == (len(nsamp), T, F)
    for b, n in enumerate(nsamp):
        Tb = rt.num_frames(n)
        if Tb:
            want = rt.fbank(x[b:b + 1, :n].contiguous())[0]
            assert want.shape[0] == Tb
            assert torch.equal(got[b, :Tb], want), (b, n)
        assert torch.count_nonzero(got[b, Tb:]) == 0
    # the forward path's feature stage (planes for the first projection) is the same front end: forward_lens == classify_lens
    rt.set_gemm_mode("f16p_stream")
    fl = [min(rt.num_frames(n), T) for n in nsamp]
    a, _ = rt.forward(x, lengths=nsamp)
    b_, _ = rt.classify(got, lengths=fl)
    assert torch.equal(a, b_)


def test_median_and_runs_lens_match_scipy_and_the_dense_calls():
    from scipy.signal import medfilt
    from uvad_amd.postprocess import labels_to_intervals, labels_to_intervals_batch, median_filter
    m, rt = _model(64)
    rng = np.random.default_rng(81)
    T = 400
    lens = [400, 1, 0, 250, 399, 49, 48, 130]
    probs = torch.from_numpy(rng.random((len(lens), T)).astype(np.float32)).cuda()
    probs[1, :] = 0.9
    k = 49
    lab = rt.median_filter(probs, k, lengths=lens)
    runs, counts = rt.label_runs(lab, lengths=lens)
    ph = probs.cpu().numpy()
    for b, L in enumerate(lens):
        if L:
            want = medfilt(np.where(ph[b, :L] < 0.5, 0, 1).astype(np.float64), k).astype(np.uint8)
            assert np.array_equal(lab[b, :L].cpu().numpy(), want), b
            dense = rt.median_filter(probs[b:b + 1, :L].contiguous(), k)
            assert torch.equal(dense[0], lab[b, :L])
            r1, c1 = rt.label_runs(dense)
            assert int(c1[0]) == int(counts[b])
            assert torch.equal(r1[0, :int(c1[0])], runs[b, :int(c1[0])])
        assert torch.count_nonzero(lab[b, L:]) == 0
    assert int(counts[2]) == 0
    # post-processing helpers with lengths (what predict_vad's ragged batches use)
    lab64 = median_filter(probs, window=0.01, lengths=lens)
    ivs = labels_to_intervals_batch(lab64, 0.01, lengths=lens)
    for b, L in enumerate(lens):
        assert ivs[b] == labels_to_intervals(lab64[b, :L].cpu().numpy(), 0.01)


def test_graph_replay_with_lengths_changed_in_place():
    F, T, B = 64, 150, 6
    m, rt = _model(F)
    feats = _feats(rt, B, T, seed=91)
    lens = torch.tensor([150, 20, 1, 0, 149, 75], dtype=torch.int32, device="cuda")
    rt.classify(feats, lengths=lens)                       # warm-up: workspace, attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _ = rt.classify(feats, lengths=lens)
    for new in ([150, 150, 150, 150, 150, 150], [3, 99, 0, 150, 42, 1], [0, 0, 0, 0, 0, 0], [200, -5, 75, 75, 1, 2]):
        lens.copy_(torch.tensor(new, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        want, _ = rt.classify(feats, lengths=[min(max(v, 0), T) for v in new])
        assert torch.equal(out, want), new


def _write_wav(path, x):
    q = np.round(x * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(q.tobytes())


def test_predict_vad_ragged_batches_give_the_predictions_of_the_default_path(tmp_path):
    from config.config import load_config
    from src.scripts import predict_vad
    from uvad_amd.synth import synth_pcm
    secs = [5.0, 40.0, 12.37, 23.5, 7.01, 31.99]
    paths = []
    for k, s in enumerate(secs):
        p = tmp_path / f"r{k}.wav"
        _write_wav(p, synth_pcm(1, int(s * 16000), seed=400 + k)[0])
        paths.append(str(p))
    cfg = load_config()
    cfg.model_dict.encoding_dim = 80
    cfg.weights_scale = 2.0
    cfg.window_seconds = None
    cfg.max_duration = 90
    cfg.input.kind = "wav"
    cfg.input.paths = paths
    want = predict_vad(**cfg)
    cfg.ragged_batches = True
    got = predict_vad(**cfg)
    assert [r["recording_id"] for r in got] == [r["recording_id"] for r in want]
    worst = 0.0
    for g, w in zip(got, want):
        assert g["num_frames"] == w["num_frames"] > 0
        assert np.array_equal(g["labels"], w["labels"]) and g["intervals"] == w["intervals"]
        worst = max(worst, float(np.abs(g["probs"] - w["probs"]).max()))
    print(f"ragged vs default: max |dprob| = {worst:.2e}")
    assert worst <= 1e-6


def test_refusals_give_their_code_and_message():
    from uvad_amd import _lib
    from uvad_amd.runtime import VadRuntime
    m, rt = _model(64)
    lib, ctx = rt.lib, rt.ctx
    feats = _feats(rt, 2, 50, seed=99)
    ws = rt.workspace(2, 50)
    out = torch.empty((2, 50), device="cuda")
    assert lib.uvad_classify_lens(ctx, feats.data_ptr(), 2, 50, None, out.data_ptr(), None, ws.data_ptr(), ws.numel(), None) == -1
    assert b"d_lens is NULL" in lib.uvad_last_error(ctx)
    pcm = torch.zeros((2, 8000), device="cuda")
    assert lib.uvad_forward_lens(ctx, pcm.data_ptr(), 2, 8000, None, out.data_ptr(), None, ws.data_ptr(), ws.numel(), None) == -1
    assert b"d_nsamp is NULL" in lib.uvad_last_error(ctx)
    assert lib.uvad_fbank_lens(ctx, pcm.data_ptr(), 2, 8000, None, out.data_ptr(), None) == -1
    assert b"d_nsamp is NULL" in lib.uvad_last_error(ctx)
    probs = torch.zeros((2, 50), device="cuda")
    lab = torch.zeros((2, 50), dtype=torch.uint8, device="cuda")
    assert lib.uvad_median_filter_lens(ctx, probs.data_ptr(), 2, 50, None, 5, lab.data_ptr(), None) == -1
    assert b"d_lens is NULL" in lib.uvad_last_error(ctx)
    assert lib.uvad_label_runs_lens(ctx, lab.data_ptr(), 2, 50, None, 4, out.data_ptr(), out.data_ptr(), None) == -1
    assert b"d_lens is NULL" in lib.uvad_last_error(ctx)
    lens = torch.tensor([50, 3], dtype=torch.int32, device="cuda")
    tiny = torch.empty(16, dtype=torch.uint8, device="cuda")
    assert lib.uvad_classify_lens(ctx, feats.data_ptr(), 2, 50, lens.data_ptr(), out.data_ptr(), None, tiny.data_ptr(), 16, None) == -4
    # no model / no tables: UVAD_E_STATE
    bare = VadRuntime(torch.device("cuda:0"), fbank=None, model=None)
    n64 = torch.tensor([8000, 100], dtype=torch.int64, device="cuda")
    assert bare.lib.uvad_classify_lens(bare.ctx, feats.data_ptr(), 2, 50, lens.data_ptr(), out.data_ptr(), None, ws.data_ptr(),
                                       ws.numel(), None) == -3
    assert b"uvad_finalize has not been called" in bare.lib.uvad_last_error(bare.ctx)
    assert bare.lib.uvad_fbank_lens(bare.ctx, pcm.data_ptr(), 2, 8000, n64.data_ptr(), out.data_ptr(), None) == -3
    assert b"uvad_set_tables has not been called" in bare.lib.uvad_last_error(bare.ctx)
    # host-side validation of list lengths
    with pytest.raises(ValueError, match=r"in \[0, 50\]"):
        rt.classify(feats, lengths=[51, 3])
    with pytest.raises(ValueError, match="2 rows"):
        rt.classify(feats, lengths=[5])
    with pytest.raises(_lib.UvadError, match="odd"):
        rt.median_filter(probs, 4, lengths=[50, 3])
