"""GPU tests (-m gpu) of int16 waveform ingest on the SincNet path (uvad_sincnet_i16 / uvad_forward_wav_i16) and of PyanNet batches kept
in flight by ForwardPipeline.

An int16 sample q means q / 32768, as on the log-mel side (uvad_fbank_i16).  The waveform kernels read int16 directly and convert
each sample as (float)q * 2^-15, the exact f32 value of q / 32768, and the waveform statistics are exact sums.  So every result here
is compared BIT FOR BIT with the f32 call on q.float() / 32768, in both forms of the conv stages (split-f16 and exact f32)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _model(seed=11, scale=4.0):
    """Seeded PyanNet: default-initialised SincNet (torch-default conv weights under `seed`), seeded classifier."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    torch.manual_seed(seed)
    m = uvad_amd.PyanNet()
    m.build()
    seed_weights(m, 1234, scale)
    return m.to(DEV).eval()


def _q(B, S, seed):
    """(B, S) int16 on the device: speech-like rows plus full-scale samples (+-32767, -32768), an all-zero row and a DC row."""
    from uvad_amd.synth import synth_pcm
    x = np.round(synth_pcm(B, S, seed=seed) * 32767.0).astype(np.int16)
    rng = np.random.default_rng(seed)
    for b in range(B):
        idx = rng.integers(0, S, size=min(S, 64))
        x[b, idx[0::3]] = 32767
        x[b, idx[1::3]] = -32767
        x[b, idx[2::3]] = -32768
    if B >= 3:
        x[1] = 0
        x[2] = 12345
    return torch.from_numpy(x).to(DEV)


def _f(q):
    return q.float() / 32768.0


@pytest.mark.parametrize("B,S", [(1, 80000), (3, 80000), (256, 80000), (1, 16000), (3, 16000), (1, 24001), (3, 24001),
                                 (1, 991 + 7), (3, 991 + 7)])
def test_int16_equals_f32_on_q_over_32768_bit_for_bit_in_both_forms(B, S):
    m = _model()
    rt = m.runtime(DEV)
    q = _q(B, S, seed=B * 100003 + S)
    for mode in ("f16p", "f32"):
        rt.set_gemm_mode(mode)
        f16 = rt.sincnet(q).clone()
        assert rt.sincnet_form() == mode
        f32 = rt.sincnet(_f(q)).clone()
        assert rt.sincnet_form() == mode
        torch.cuda.synchronize()
        assert f16.shape == (B, rt.sincnet_num_frames(S), 60)
        assert torch.isfinite(f16).all()
        assert torch.equal(f16, f32), (mode, (f16 - f32).abs().max().item())
        l16, p16 = (t.clone() for t in rt.forward_wav(q))
        assert rt.sincnet_form() == mode
        l32, p32 = rt.forward_wav(_f(q))
        torch.cuda.synchronize()
        assert torch.equal(l16, l32) and torch.equal(p16, p32), mode
    rt.set_gemm_mode("f16p")
    # the module tree passes int16 through unchanged: (batch, channel, samples) as the reference's PyanNet takes it
    logits, _ = m.forward_logits(q.unsqueeze(1))
    assert torch.equal(logits, rt.forward_wav(_f(q))[0])
    assert torch.equal(m(q.unsqueeze(1)), m(_f(q).unsqueeze(1)))


@pytest.mark.parametrize("S", [16000, 24001])
def test_int16_rows_read_nothing_outside_themselves_and_misaligned_rows_match(S):
    """Poison rows: the B rows handed over sit between two rows of +-32767 in one allocation; an out-of-row read of the 16-byte load
    path or of the scalar tail would change the edge frames.  Misaligned rows: a view starting at element 1 (2 bytes off the 16-byte
    boundary), S odd for the later rows, so the vector loads are off and the scalar path runs.  Every result equals the f32 call on
    the same samples, in both forms."""
    m = _model(seed=23)
    rt = m.runtime(DEV)
    B = 4
    body = _q(B, S, seed=S)
    for mode in ("f16p", "f32"):
        rt.set_gemm_mode(mode)
        want_f = rt.sincnet(_f(body)).clone()
        want_l = rt.forward_wav(_f(body))[0].clone()
        for poison in (32767, -32767):
            buf = torch.full((B + 2, S), poison, dtype=torch.int16, device=DEV)
            buf[1:B + 1] = body
            v = buf[1:B + 1]
            assert v.is_contiguous()
            assert torch.equal(rt.sincnet(v), want_f), (mode, poison)
            assert rt.sincnet_form() == mode
            assert torch.equal(rt.forward_wav(v)[0], want_l), (mode, poison)
        flat = torch.full((B * S + 9,), 32767, dtype=torch.int16, device=DEV)
        flat[1:1 + B * S] = body.reshape(-1)
        mis = flat[1:1 + B * S].view(B, S)
        assert mis.data_ptr() % 16 == 2
        assert torch.equal(rt.sincnet(mis), want_f), mode
        assert torch.equal(rt.forward_wav(mis)[0], want_l), mode
    rt.set_gemm_mode("f16p")


def test_forward_wav_i16_replayed_from_a_hipgraph_equals_the_eager_call():
    m = _model(seed=17)
    rt = m.runtime(DEV)
    q = _q(6, 40000, seed=21)
    for mode in ("f16p", "f32"):
        rt.set_gemm_mode(mode)
        side = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(side):
            eager, eager_p = (t.clone() for t in rt.forward_wav(q))            # (also sizes the workspace outside the capture)
            form = rt.sincnet_form()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                cap, cap_p = rt.forward_wav(q)
        assert form == mode
        cap.zero_(); cap_p.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, eager) and torch.equal(cap_p, eager_p), mode
        assert torch.equal(eager, rt.forward_wav(_f(q))[0]), mode
    rt.set_gemm_mode("f16p")


def test_forward_pipeline_runs_pyannet_batches_with_the_bits_of_the_sequential_path():
    """ForwardPipeline(PyanNet): its slots run uvad_forward_wav[_i16]; each batch's logits equal a sequential forward_wav with the same
    recurrent form, for int16 and f32 batches mixed.  Depth <= 3: the test machines default to four hardware queues."""
    import uvad_amd
    from uvad_amd.synth import synth_pcm_device
    m = _model(seed=31)
    rt = m.runtime(DEV)
    batches = [_q(24, 48000, seed=70 + i) if i % 2 == 0 else synth_pcm_device(24, 48000, 70 + i, DEV) for i in range(5)]
    assert {b.dtype for b in batches} == {torch.int16, torch.float32}
    want = [rt.forward_wav(b)[0].clone() for b in batches]
    pipe = uvad_amd.ForwardPipeline(m, DEV, depth=2)
    try:
        got = [p.result()[0] for p in [pipe.submit(b) for b in batches]]
        assert len(pipe.streams) == 2 and pipe.streams[0] != pipe.streams[1]
        for w, g in zip(want, got):
            assert torch.equal(w, g)
    finally:
        pipe.close()
    rt.set_recurrent_tile(16)
    want16 = [tuple(t.clone() for t in rt.forward_wav(b)) for b in batches]
    rt.set_recurrent_tile(0)
    pipe = uvad_amd.ForwardPipeline(m, DEV, depth=3, recurrent_tile=16)
    try:
        pend = [pipe.submit(b, want_probs=True) for b in batches]
        got16 = [p.result() for p in pend]
        assert all(r.recurrent_tile() == 16 for r in pipe.runtimes)
        for (w, wp), (g, gp) in zip(want16, got16):
            assert torch.equal(w, g) and torch.equal(wp, gp)
    finally:
        pipe.close()
    with pytest.raises(RuntimeError, match="attach_fbank"):
        m2 = uvad_amd.PyanNet2(encoding_dim=64)
        m2.build()
        uvad_amd.ForwardPipeline(m2, DEV)


def test_predict_vad_sincnet_sends_int16_batches_through_a_pipeline_with_unchanged_predictions(tmp_path, monkeypatch):
    """predict_vad(feature_extractor="sincnet") on int16 wav files, max_duration forcing several batches plus a kept tail: a pipeline is
    opened, the batches reach it as int16, and the predictions equal the sequential fallback (streams that never overlap) and, window by
    window, PyanNet on q.float() / 32768 with the tail zero-padded to 5 s."""
    import wave
    import uvad_amd
    from uvad_amd import scripts
    from uvad_amd.runtime import VadRuntime
    from uvad_amd.synth import synth_pcm
    from config.config import load_config
    monkeypatch.setenv("UVAD_FEATURE_EXTRACTOR", "sincnet")
    lens = {"a.wav": int(23.7 * 16000), "b.wav": 12 * 16000}
    pcm = {}
    for k, (name, n) in enumerate(lens.items()):
        q = np.round(synth_pcm(1, n, seed=900 + k)[0] * 32767.0).astype("<i2")
        pcm[name] = q
        with wave.open(str(tmp_path / name), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(q.tobytes())

    opened, dtypes = [], []

    class Spy(uvad_amd.ForwardPipeline):
        def __init__(self, model, *a, **k):
            opened.append(model)
            super().__init__(model, *a, **k)

        def submit(self, pcm, *a, **k):
            dtypes.append(pcm.dtype)
            return super().submit(pcm, *a, **k)

    monkeypatch.setattr(scripts, "ForwardPipeline", Spy)

    def run():
        cfg = load_config()
        cfg.input.kind = "wav"
        cfg.input.paths = [str(tmp_path / n) for n in lens]
        cfg.max_duration = 10          # two 5 s cuts per batch: 3 batches of full cuts + the kept 3.7 s tail
        return {r["recording_id"]: r for r in scripts.predict_vad(**cfg)}

    got = run()
    assert len(opened) == 1 and isinstance(opened[0], uvad_amd.PyanNet)
    assert dtypes == [torch.int16] * 4
    net = opened[0]
    monkeypatch.setattr(VadRuntime, "streams_overlap", lambda self, a, b: False)
    seq = run()
    assert len(dtypes) == 4                                                  # nothing was submitted to a pipeline the second time
    for name in lens:
        g, s = got[name], seq[name]
        assert g["num_frames"] == s["num_frames"] > 0
        assert np.array_equal(g["labels"], s["labels"]) and np.array_equal(g["probs"], s["probs"]) and g["intervals"] == s["intervals"]
    # window by window against PyanNet on the f32 signal q / 32768 (tail padded with zeros to 80 000 samples)
    for name, n in lens.items():
        q = pcm[name]
        k = 0
        for st in range(0, n, 80000):
            ln = min(80000, n - st)
            if ln <= 48000:
                continue
            win = np.zeros(80000, np.int16)
            win[:ln] = q[st:st + ln]
            _, want = net.forward_logits(_f(torch.from_numpy(win).to(DEV))[None], want_logits=False)
            row = got[name]["probs"][k * 293:(k + 1) * 293]
            assert len(row) > 0 and np.array_equal(row, want[0].cpu().numpy()[:len(row)]), (name, k)
            k += 1
        assert k * 293 >= got[name]["num_frames"] > (k - 1) * 293


def test_int16_errors_are_the_f32_errors():
    m = _model()
    rt = m.runtime(DEV)
    for call in (rt.sincnet, rt.forward_wav):
        for dtype in (torch.float32, torch.int16):
            with pytest.raises(RuntimeError, match=r"wav must be a tensor on cuda:0 \(got cpu\)"):
                call(torch.zeros(1, 16000, dtype=dtype))
            with pytest.raises(ValueError, match="700 samples are too short for one SincNet frame"):
                call(torch.zeros(1, 700, dtype=dtype, device=DEV))
