"""GPU tests (-m gpu) of the ingest stage (uvad_ingest*, VadRuntime.ingest*): G.711 / int16 / f32 sources, interleaved channels to rows,
polyphase resampling to 16 kHz, in its dense, ragged and stream forms, alone and in front of the served models.

  identity   int16 at 16 kHz is x / 32768 bit for bit, and forward(ingest(x)) is forward_i16(x) bit for bit, both models
  decode     every mu-law / A-law code of every channel equals audioop's expansion / 32768 bit for bit
  accuracy   every output sample within the DERIVED bound of the float64 evaluation on the same f32 taps (tests/ingest_ref.py):
             (K + 1) 2^-24 sum_k |taps[p][k]| max|x| -- a length-K f32 fma chain on exactly representable inputs
  ragged     a row equals the dense ingest of its prefix alone; +0 past its count; NaN padding never read; the counts drive forward()
  stream     the concatenated steps equal the dense output delayed by D, bit for bit, eager and from one captured graph
  slots      UVAD_SLOT_START restarts one row and leaves its neighbours' bits alone
  served     512 feeds x 20 ms of 8 kHz mu-law through both slot pools equal the pools fed the dense-ingested, D-shifted audio
  predict    predict_vad on an 8 kHz two-channel mu-law file, channels "all" / "first"; a 16 kHz int16 file keeps today's path
"""
import audioop

import numpy as np
import pytest
import torch

import ingest_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TORCH_DT = {"f32": torch.float32, "int16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


def _rt():
    from uvad_amd.runtime import VadRuntime
    return VadRuntime(DEV)


def _source(encoding, shape, seed):
    """Random source samples in the encoding (numpy): speech-like int16 for the linear types, their G.711 codes for the others."""
    from uvad_amd.synth import synth_pcm
    B = int(np.prod(shape[:1]))
    n = int(np.prod(shape[1:]))
    x = synth_pcm(B, max(n, 1), seed=seed)[:, :n].reshape(shape)
    q = np.round(x * 32767.0).astype(np.int16)
    if encoding == "f32":
        return (q.astype(np.float32) / np.float32(32768.0))
    if encoding == "int16":
        return q
    fn = audioop.lin2ulaw if encoding == "ulaw" else audioop.lin2alaw
    return np.frombuffer(fn(q.astype("<i2").tobytes(), 2), np.uint8).reshape(shape).copy()


def _logmel(F=64, scale=2.0):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet2(lstm={"bidirectional": True}, encoding_dim=F)
    m.build()
    seed_weights(m, 1234, scale)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type="povey"))
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


def _wavmodel(seed=11, scale=2.0):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    torch.manual_seed(seed)
    m = uvad_amd.PyanNet()
    m.build()
    seed_weights(m, 1234, scale)
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. identity

def test_int16_16k_is_the_pure_decode_and_feeds_both_models_the_same_bits():
    x = torch.from_numpy(_source("int16", (3, 40000), seed=1)).to(DEV)
    m, rt = _logmel()
    plan = rt.ingest_configure("int16", 1, 16000)
    assert (plan["up"], plan["down"], plan["delay"]) == (1, 1, 0)
    y = rt.ingest(x)
    assert y.dtype == torch.float32 and torch.equal(y, x.float() / 32768)
    for a, b in zip(rt.forward(y), rt.forward(x)):
        assert torch.equal(a, b)
    mw, rtw = _wavmodel()
    rtw.ingest_configure("int16", 1, 16000)
    yw = rtw.ingest(x)
    assert torch.equal(yw, y)
    for a, b in zip(rtw.forward_wav(yw), rtw.forward_wav(x)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. decode and channels

@pytest.mark.parametrize("encoding", ["ulaw", "alaw"])
def test_g711_two_channels_equal_audioop_bit_for_bit(encoding):
    rt = _rt()
    rt.ingest_configure(encoding, 2, 16000)
    B, S = 3, 5003
    raw = np.random.default_rng(7).integers(0, 256, (B, S, 2)).astype(np.uint8)
    raw[0, :256, 0] = np.arange(256)                           # every code, both channels
    raw[0, :256, 1] = np.arange(255, -1, -1)
    y = rt.ingest(torch.from_numpy(raw).to(DEV)).cpu().numpy()
    assert y.shape == (B * 2, S)
    for b in range(B):
        for c in range(2):
            want = ref.decode(raw[b, :, c], encoding).astype(np.float32)
            assert np.array_equal(y[b * 2 + c].view(np.uint32), want.view(np.uint32)), (b, c)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. resampler accuracy

@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("encoding", ["int16", "ulaw"])
@pytest.mark.parametrize("rate", [8000, 24000, 32000, 48000])
def test_every_sample_within_the_derived_bound_of_float64(rate, encoding, channels):
    from uvad_amd.ingest import resample_taps
    rt = _rt()
    plan = rt.ingest_configure(encoding, channels, rate)
    taps, up, down, width = resample_taps(rate)
    K = taps.shape[1]
    rng = np.random.default_rng(rate + channels)
    lengths = [1, 2, 3, width, K - 1, K, K + 1, 37] + rng.integers(K, 9000, 5).tolist() + [4096, 12289]   # shorter than the filter too
    worst = 0.0
    for n in lengths:
        raw = _source(encoding, (2, n, channels), seed=rate // 1000 + n)
        y = rt.ingest(torch.from_numpy(raw).to(DEV)).cpu().numpy().astype(np.float64)
        m = ref.out_len(n, up, down)
        assert y.shape == (2 * channels, m), (n, y.shape)                # the output length is exact
        for b in range(2):
            for c in range(channels):
                x = ref.decode(raw[b, :, c], encoding)
                want = ref.resample_f64(x, taps, up, down, width)
                bound = ref.chain_bound(taps, np.abs(x).max())[np.arange(m) % up]
                err = np.abs(y[b * channels + c] - want)                  # every sample: none is left out
                assert err.shape == (m,) and (err <= bound).all(), (n, b, c, float(err.max()), float(bound.max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"{rate} Hz {encoding} x{channels}: delay {plan['delay']}, worst error / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. ragged

@pytest.mark.parametrize("rate,channels", [(8000, 2), (48000, 1), (16000, 2)])
def test_ragged_rows_are_their_prefixes_alone_and_padding_is_never_read(rate, channels):
    rt = _rt()
    plan = rt.ingest_configure("f32", channels, rate)
    up, down = plan["up"], plan["down"]
    B, S = 7, 6001
    lens = [0, 1, 5, 2999, 3000, 6000, S]
    raw = _source("f32", (B, S, channels), seed=rate // 100)
    dirty = raw.copy()
    for b, n in enumerate(lens):
        dirty[b, n:] = np.nan                                   # poisoned padding
    y, cnt = rt.ingest(torch.from_numpy(dirty).to(DEV), lengths=lens)
    y2, cnt2 = rt.ingest(torch.from_numpy(raw).to(DEV), lengths=torch.tensor(lens, device=DEV))
    assert cnt.dtype == torch.int64 and cnt.tolist() == [ref.out_len(n, up, down) for n in lens for _ in range(channels)]
    assert torch.equal(cnt, cnt2) and torch.equal(y.view(torch.int32), y2.view(torch.int32))
    assert not torch.isnan(y).any()
    for b, n in enumerate(lens):
        m = ref.out_len(n, up, down)
        alone = rt.ingest(torch.from_numpy(raw[b:b + 1, :n]).to(DEV))
        assert alone.shape == (channels, m)
        for c in range(channels):
            row = y[b * channels + c]
            assert torch.equal(row[:m].view(torch.int32), alone[c].view(torch.int32)), (b, c)
            assert (row[m:].view(torch.int32) == 0).all(), (b, c)                  # +0, not -0


def test_emitted_counts_drive_forward_to_the_bits_of_per_row_calls():
    m, rt = _logmel()
    rt.set_gemm_mode("f32")
    rt.set_recurrent_tile(4)
    rt.ingest_configure("ulaw", 2, 8000)
    B, S = 3, 20000
    lens = [20000, 8123, 15000]
    raw = _source("ulaw", (B, S, 2), seed=91)
    y, cnt = rt.ingest(torch.from_numpy(raw).to(DEV), lengths=lens)
    lg, pr = rt.forward(y, lengths=cnt)
    for r in range(B * 2):
        n = int(cnt[r])
        T = rt.num_frames(n)
        lg1, pr1 = rt.forward(y[r:r + 1, :n].contiguous())
        assert torch.equal(lg[r, :T], lg1[0]) and torch.equal(pr[r, :T], pr1[0]), r
        assert (lg[r, T:] == 0).all() and (pr[r, T:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. stream equals batch

def _stream_all(rt, raw, chunk_in, graphs=False, flags=None):
    B = raw.shape[0]
    st = rt.ingest_open(B, chunk_in, graphs=graphs)
    x = torch.from_numpy(raw).to(DEV)
    outs = []
    for s in range(raw.shape[1] // chunk_in):
        start = None if flags is None or not flags[s].any() else flags[s].astype(bool)
        outs.append(rt.ingest_step(st, x[:, s * chunk_in:(s + 1) * chunk_in], start=start).clone())
    return torch.cat(outs, 1), st


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("encoding", ["f32", "int16", "ulaw"])
@pytest.mark.parametrize("rate,ms", [(8000, 10), (8000, 20), (8000, 30), (48000, 20), (24000, 30), (8000, 500)])
def test_stream_is_the_dense_output_delayed_by_D_bit_for_bit(rate, ms, encoding, channels):
    rt = _rt()
    plan = rt.ingest_configure(encoding, channels, rate)
    D = plan["delay"]
    chunk_in = rate * ms // 1000
    steps = 12 if ms < 500 else 3
    raw = _source(encoding, (3, steps * chunk_in, channels), seed=rate // 1000 + ms)
    dense = rt.ingest(torch.from_numpy(raw).to(DEV))
    got, _ = _stream_all(rt, raw, chunk_in)
    N = dense.shape[1]
    assert got.shape == dense.shape and D == ref.delay(plan["up"], plan["down"], plan["width"]) and 0 < D < N
    assert (got[:, :D].view(torch.int32) == 0).all()                                    # D leading +0
    assert torch.equal(got[:, D:].view(torch.int32), dense[:, :N - D].view(torch.int32))
    replay, st = _stream_all(rt, raw, chunk_in, graphs=True)
    assert st["graphs"] == 1                                                              # one captured graph served every step
    assert torch.equal(replay.view(torch.int32), got.view(torch.int32))


def test_replaying_the_captured_step_allocates_nothing_and_never_synchronises():
    rt = _rt()
    rt.ingest_configure("ulaw", 1, 8000)
    B, chunk_in = 512, 160
    raw = _source("ulaw", (B, 8 * chunk_in, 1), seed=5)
    x = torch.from_numpy(raw).to(DEV)
    st = rt.ingest_open(B, chunk_in, graphs=True)
    rt.ingest_step(st, x[:, :chunk_in])
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(50):
            st["graph"].replay()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before and st["graphs"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. slots

def test_slot_start_restarts_one_row_and_leaves_its_neighbours_alone():
    rt = _rt()
    plan = rt.ingest_configure("ulaw", 2, 8000)
    B, chunk_in, steps, at = 3, 160, 14, 5
    co = chunk_in * plan["up"] // plan["down"]
    raw = _source("ulaw", (B, steps * chunk_in, 2), seed=23)
    plain, _ = _stream_all(rt, raw, chunk_in)
    flags = np.zeros((steps, B * 2), np.uint8)
    flags[at, 4] = 1                                            # source row 2, channel 0
    got, _ = _stream_all(rt, raw, chunk_in, flags=flags)
    others = [r for r in range(B * 2) if r != 4]
    assert torch.equal(got[others].view(torch.int32), plain[others].view(torch.int32))
    assert torch.equal(got[4, :at * co].view(torch.int32), plain[4, :at * co].view(torch.int32))
    fresh, _ = _stream_all(rt, raw[2:3, at * chunk_in:], chunk_in)
    assert torch.equal(got[4, at * co:].view(torch.int32), fresh[0].view(torch.int32))
    assert not torch.equal(got[4, at * co:at * co + 2 * plan["delay"]], plain[4, at * co:at * co + 2 * plan["delay"]])
    replay, st = _stream_all(rt, raw, chunk_in, graphs=True, flags=flags)
    assert st["graphs"] == 1 and torch.equal(replay.view(torch.int32), got.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 12. through the served models at the named serving size

def _churn(B, steps, seed):
    rng = np.random.default_rng(seed)
    f = np.zeros((steps, B), np.uint8)
    f[0, 0] = 1
    f[5, 1] = f[steps // 2, 1] = 3
    f[3, 2], f[8, 2] = 1, 2
    f[2, 3], f[10, 3], f[steps - 5, 3] = 1, 1, 2
    for b in range(4, B - 1):
        live = False
        for s in range(1 + b % 7, steps):
            r = rng.random()
            if not live and r < 0.12:
                f[s, b] = 3 if rng.random() < 0.15 else 1
                live = f[s, b] == 1
            elif live and r < 0.03:
                f[s, b] = 1                                     # START on a busy slot
            elif live and r < 0.07:
                f[s, b], live = 2, False
    return f


def _sessions(flags):
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


@pytest.mark.parametrize("family", ["wav", "logmel"])
def test_512_feeds_of_8k_ulaw_through_the_slot_pools_equal_the_dense_ingested_shifted_audio(family):
    B, chunk_in, steps = 512, 160, 110
    if family == "wav":
        m, rt = _wavmodel()
        W, L = 293, 30
        open_pool = lambda: rt.wav_window_slots_open(B, 320, window=W, lookahead=L, graphs=True, dtype=torch.float32)
        step_pool = rt.wav_window_slots_step
    else:
        m, rt = _logmel()
        W, L = 200, 10
        open_pool = lambda: rt.window_slots_open(B, 320, window=W, lookahead=L, graphs=True)
        step_pool = rt.window_slots_step
    plan = rt.ingest_configure("ulaw", 1, 8000)
    D, co = plan["delay"], 320
    flags = _churn(B, steps, seed=512)
    raw = _source("ulaw", (B, steps * chunk_in, 1), seed=77)
    x = torch.from_numpy(raw).to(DEV)
    # the reference feed: every session dense-ingested on its own (one ragged call), shifted by D into the session's steps
    sess = _sessions(flags)
    longest = max(s1 - s0 + 1 for _, s0, s1 in sess) * chunk_in
    xs = np.zeros((len(sess), longest, 1), np.uint8)
    for i, (b, s0, s1) in enumerate(sess):
        xs[i, :(s1 - s0 + 1) * chunk_in] = raw[b, s0 * chunk_in:(s1 + 1) * chunk_in]
    y, cnt = rt.ingest(torch.from_numpy(xs).to(DEV), lengths=[(s1 - s0 + 1) * chunk_in for _, s0, s1 in sess])
    z = torch.zeros((B, steps * co), device=DEV)
    cnt = cnt.tolist()
    for i, (b, s0, s1) in enumerate(sess):
        n = (s1 - s0 + 1) * co
        assert cnt[i] == n
        z[b, s0 * co + D:s0 * co + n] = y[i, :n - D]
    ing = rt.ingest_open(B, chunk_in, graphs=True)
    fed, shifted = open_pool(), open_pool()
    emitted = 0
    for s in range(steps):
        fl = flags[s]
        st, en = (fl & 1 == 1), (fl & 2 == 2)
        a = rt.ingest_step(ing, x[:, s * chunk_in:(s + 1) * chunk_in], start=st if st.any() else None)
        lg1, c1 = step_pool(fed, a, start=st, end=en)
        lg1, c1 = lg1.clone(), c1.clone()
        lg2, c2 = step_pool(shifted, z[:, s * co:(s + 1) * co], start=st, end=en)
        assert torch.equal(c1, c2), s
        cols = torch.arange(lg1.shape[1], device=DEV)[None, :] < c1[:, None]
        assert torch.equal(lg1[cols].view(torch.int32), lg2[cols].view(torch.int32)), s
        emitted += int(c1.sum())
    assert ing["graphs"] == 1 and fed["graphs"] == 1 and emitted > 0
    print(f"{family}: {steps} steps x {B} feeds, {len(sess)} sessions, {emitted} frames emitted, bitwise")


# ---------------------------------------------------------------------------------------------------------------------------------
# 13. predict_vad

def _predict_cfg(paths, channels=None):
    from config.config import load_config
    cfg = load_config()
    cfg.model_dict.encoding_dim = 80
    cfg.weights_scale = 2.0
    cfg.max_duration = 90
    cfg.input.kind = "wav"
    cfg.input.paths = paths
    if channels is not None:
        cfg.input.channels = channels
    return cfg


def _predict_model(cfg):
    """The model predict_vad builds from cfg (seeded weights), and its runtime."""
    from uvad_amd.engine import VadModel
    from uvad_amd.features import FbankConfig
    from uvad_amd.synth import seed_weights
    torch.manual_seed(cfg["seed"])
    model = VadModel(model_name=cfg["model_name"], model_dict=dict(cfg["model_dict"]))
    seed_weights(model.model, cfg.get("weights_seed", 1234), cfg.get("weights_scale", 4.0))
    net = model.to(DEV).eval().model
    net.attach_fbank(FbankConfig(sampling_rate=16000, num_filters=net.encoding_dim, window_type=cfg.get("window_type", "povey"),
                                 frame_shift=cfg["frame_shift"], device="cuda"))
    return net, net.runtime(DEV)


def test_predict_vad_8k_two_channel_ulaw_file(tmp_path):
    from uvad_amd.scripts import predict_vad
    raw = _source("ulaw", (1, 88000, 2), seed=31)[0]                                  # 11 s at 8 kHz, two channels
    p = str(tmp_path / "call.wav")
    ref.write_wav(p, raw, 7, 8000)
    cfg = _predict_cfg([p], "all")
    got = {r["recording_id"]: r for r in predict_vad(**cfg)}
    assert sorted(got) == ["call.wav-ch0", "call.wav-ch1"]
    net, rt = _predict_model(cfg)
    rt.ingest_configure("ulaw", 2, 8000)
    y = rt.ingest(torch.from_numpy(raw[None]).to(DEV))                                # (2, 176000)
    assert y.shape == (2, 176000)
    wins = lambda rows: torch.stack([y[c, w * 80000:(w + 1) * 80000] for c in rows for w in range(2)])   # 5 s cuts; the 1 s tail is dropped
    _, pr = rt.forward(wins([0, 1]), want_logits=False)
    for c in range(2):
        r = got[f"call.wav-ch{c}"]
        want = torch.cat([pr[2 * c], pr[2 * c + 1]]).cpu().numpy()
        assert r["num_frames"] == 1000 and np.array_equal(r["probs"].view(np.uint32), want[:1000].view(np.uint32)), c
        assert all(0.0 <= a < b <= 11.0 for a, b in r["intervals"])                     # seconds of the recording, as before
    only = predict_vad(**_predict_cfg([p]))
    assert [r["recording_id"] for r in only] == ["call.wav"]
    _, pr0 = rt.forward(wins([0]), want_logits=False)
    assert np.array_equal(only[0]["probs"].view(np.uint32), torch.cat([pr0[0], pr0[1]]).cpu().numpy()[:1000].view(np.uint32))
    with pytest.raises(ValueError, match="'first' or 'all'"):
        predict_vad(**_predict_cfg([p], "mix"))


def test_predict_vad_16k_int16_mono_file_keeps_todays_path(tmp_path, monkeypatch):
    import wave
    from uvad_amd.runtime import VadRuntime
    from uvad_amd.scripts import predict_vad
    q = _source("int16", (1, 160000), seed=32)[0]
    p = str(tmp_path / "plain.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(q.astype("<i2").tobytes())
    called = []
    monkeypatch.setattr(VadRuntime, "ingest", lambda self, *a, **k: called.append(1) or (_ for _ in ()).throw(AssertionError("ingest called")))
    cfg = _predict_cfg([p])
    (r,) = predict_vad(**cfg)
    assert not called and r["recording_id"] == "plain.wav"
    net, rt = _predict_model(cfg)
    x = torch.from_numpy(q.reshape(2, 80000)).to(DEV)
    _, pr = rt.forward(x, want_logits=False)                                            # int16: uvad_forward_i16
    assert np.array_equal(r["probs"].view(np.uint32), torch.cat([pr[0], pr[1]]).cpu().numpy()[:r["num_frames"]].view(np.uint32))
