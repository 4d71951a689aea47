"""GPU tests (-m gpu) of the ingest stage where tests/test_gpu_ingest.py does not look: every resampling ratio the tap limits admit, 3 to 8
channels, tiles shrunk to fit LDS, uploaded tables whose every tap carries weight, the limits themselves, stream chunks shorter than
the history.  The helpers and the shared cases are in tests/ingest_ref.py; tests/test_ingest_ref.py shows on the CPU that the derived
bound holds for the kernel's arithmetic on exactly these inputs.

  designed   13 rates of the general phase loop (up in {4, 5, 8}) and of 40 / 64 kHz, 1 / 3 / 8 channels, int16 / mu-law / f32: one ragged
             call per case with rows on every tile edge; every sample within the derived bound of float64, counts, +0 past them, rows
             bit-equal to the dense ingest of their prefix alone
  tables     the same with random full-weight tables: 8 phases, 64 taps, K = down (width 0), for each kernel instantiation
  impulse    one sample of 0.5 in an otherwise zero row: the output IS the table, bit for bit, zero elsewhere -- no tolerance
  shrink     8 channels at 48 / 64 / 40 / 32 kHz (tiles halved to fit 48 KiB) and 5 channels at 12 kHz, dense
  stream     equals the dense output delayed by D, bit for bit, eager and from one captured graph: general ratios, a shrunken tile 0
             beside a history, several tiles per step, one output group per step (chunk shorter than the history), long histories
  slots      UVAD_SLOT_START on the general path: neighbours untouched, the restarted row a fresh stream, held groups included
  predict    predict_vad on a 12 kHz three-channel int16 file
"""
import numpy as np
import pytest
import torch

import ingest_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_ID = lambda k: f"{k[0]}-{k[1]}-x{k[2]}"   # noqa: E731


def _rt():
    from uvad_amd.runtime import VadRuntime
    return VadRuntime(DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.view(torch.int32)


def _instantiation(up):
    return f"ingest_kernel<{up if up in (1, 2) else 0}>"


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2. accuracy against float64, one ragged call per case

def _accuracy(key, custom):
    case = ref.accuracy_case(key)
    up, down, width, K, Cn, enc = case["up"], case["down"], case["width"], case["K"], case["channels"], case["encoding"]
    rt = _rt()
    plan = rt.ingest_configure(enc, Cn, case["rate"], taps=case["taps"] if custom else None)
    assert (plan["up"], plan["down"], plan["width"]) == (up, down, width)
    lens, raw = case["lengths"], case["raw"]
    x = _dev(raw)
    y, cnt = rt.ingest(x, lengths=lens)
    counts = [ref.out_len(n, up, down) for n in lens]
    assert y.shape == (len(lens) * Cn, ref.out_len(max(lens), up, down))
    assert cnt.tolist() == [m for m in counts for _ in range(Cn)]                          # counts equal out_len
    yh = y.cpu().numpy()
    worst = ref.check_rows(case, lambda b, c: yh[b * Cn + c])                              # every sample of every row
    for b, m in enumerate(counts):
        assert (yh[b * Cn:(b + 1) * Cn, m:].view(np.uint32) == 0).all(), b                  # +0 past the count, not -0
    subset = sorted(set(range(1, len(lens), 3)) | {len(lens) - 1})
    for b in subset:                                                                       # a row is the dense ingest of its prefix alone
        n, m = lens[b], counts[b]
        if n == 0:
            continue
        alone = rt.ingest(x[b:b + 1, :n].contiguous())
        assert alone.shape == (Cn, m)
        assert torch.equal(_bits(alone), _bits(y[b * Cn:(b + 1) * Cn, :m])), (b, n)
    print(f"{key[0]} {enc} x{Cn}: {up}/{down} K {K} {_instantiation(up)} TJ {case['TJ']} rows {len(lens)} S_out % 4 = {y.shape[1] % 4}, "
          f"worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("key", ref.DESIGNED_CASES, ids=_ID)
def test_designed_tables_every_sample_within_the_derived_bound_of_float64(key):
    _accuracy(key, custom=False)


@pytest.mark.parametrize("key", ref.TABLE_CASES, ids=_ID)
def test_random_full_weight_tables_every_sample_within_the_derived_bound_of_float64(key):
    _accuracy(key, custom=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. impulse response equals the table, bit for bit

def _impulse_source(encoding, shape):
    return np.zeros(shape, np.int16 if encoding == "int16" else np.float32)


def _check_impulses(y, where, taps, up, down, width, n_out, shift=0):
    """y numpy (rows, n_out); where: {row: frame of its impulse}; every other row, and every output off an impulse's support, is zero."""
    for r in range(y.shape[0]):
        if r not in where:
            assert (y[r] == 0).all(), r
            continue
        want, mask = ref.impulse_response(taps, up, down, width, where[r], n_out, shift)
        assert mask.any() or shift, (r, where[r])                                            # (a stream never emits its last D samples)
        assert np.array_equal(y[r][mask].view(np.uint32), want[mask].view(np.uint32)), (r, where[r])   # the table's bits
        assert (y[r][~mask] == 0).all(), (r, where[r])


@pytest.mark.parametrize("channels", [3, 8])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])                                  # <0> with 8 phases, <0> with up = 5 at 64 taps, <1>, <2>
def test_impulse_response_is_the_table_bit_for_bit(name, channels):
    taps, rate, up, down, width = ref.table(name)
    K = taps.shape[1]
    TJ = ref.tiling(up, down, K, channels)
    n = 3 * TJ * down + 5                                                                # three whole tiles and the head of a fourth
    frames = ref.impulse_frames(TJ, down, width, K, n)
    assert len(frames) >= 16 and frames[0] == 0 and frames[1] == n - 1
    B = -(-len(frames) // channels) + 1                                                  # one impulse per (row, channel); the last row has none
    n_out = ref.out_len(n, up, down)
    rt = _rt()
    for enc in ("int16", "f32"):
        rt.ingest_configure(enc, channels, rate, taps=taps)
        raw = _impulse_source(enc, (B, n, channels))
        slots = np.random.default_rng(n + channels).permutation((B - 1) * channels)[:len(frames)]   # scattered over rows and channels
        where = {int(r): m for r, m in zip(slots, frames)}
        for r, m in where.items():
            raw[r // channels, m, r % channels] = 16384 if enc == "int16" else 0.5
        y = rt.ingest(_dev(raw)).cpu().numpy()
        assert y.shape == (B * channels, n_out)
        _check_impulses(y, where, taps, up, down, width, n_out)
    print(f"table {name} x{channels}: {up}/{down} K {K} {_instantiation(up)} TJ {TJ}, {len(frames)} impulses, every output checked, bitwise")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. tiles shrunk to fit LDS

@pytest.mark.parametrize("rate,channels", [(48000, 8), (64000, 8), (40000, 8), (32000, 8), (12000, 5)])
def test_many_channels_shrunken_tiles_within_the_derived_bound(rate, channels):
    from uvad_amd.ingest import resample_taps
    taps, up, down, width = resample_taps(rate)
    K = taps.shape[1]
    TJ, whole = ref.tiling(up, down, K, channels), ref.tiling(up, down, K, 1)
    print(f"{rate} Hz x{channels}: {up}/{down} K {K} {_instantiation(up)} TJ {TJ} (one channel: {whole})")
    assert whole == ref._round4(-(-ref.TILE_OUT // up))
    if channels == 8:
        assert TJ < whole                                                                # the case still covers the shrink
    rt = _rt()
    rt.ingest_configure("int16", channels, rate)
    worst = 0.0
    long, edge = -(-(3 * whole * up + 9) * down // up), 2 * TJ * down + 1               # (2 TJ down frames end on the edge of tile 1)
    assert ref.out_len(long, up, down) > 3 * whole * up                                  # at least 3 unshrunken tiles
    past = ref.out_len(edge, up, down) - 2 * TJ * up                                     # the least count past a (shrunken) tile's edge:
    assert past == (1 if up <= down else -(-up // down)), past                           # one sample wherever up / down can produce it
    for n in (long, edge):
        m = ref.out_len(n, up, down)
        raw = ref.random_source("int16", (2, n, channels), seed=rate + n)
        y = rt.ingest(_dev(raw)).cpu().numpy().astype(np.float64)
        assert y.shape == (2 * channels, m)
        for b in range(2):
            for c in range(channels):
                x = ref.decode(raw[b, :, c], "int16")
                want = ref.resample_f64(x, taps, up, down, width)
                bound = ref.chain_bound(taps, np.abs(x).max())[np.arange(m) % up]
                err = np.abs(y[b * channels + c] - want)                                  # every sample
                assert err.shape == (m,) and (err <= bound).all(), (n, b, c, float(err.max()), float(bound.max()))
                worst = max(worst, float((err / bound).max()))
    print(f"{rate} Hz x{channels}: worst error / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. stream equals dense delayed by D

def _stream_all(rt, raw, chunk_in, graphs=False, flags=None):
    st = rt.ingest_open(raw.shape[0], chunk_in, graphs=graphs)
    x = _dev(raw)
    outs = []
    for s in range(raw.shape[1] // chunk_in):
        start = None if flags is None or not flags[s].any() else flags[s].astype(bool)
        outs.append(rt.ingest_step(st, x[:, s * chunk_in:(s + 1) * chunk_in], start=start).clone())
    return torch.cat(outs, 1), st


def _stream_equals_dense(rt, plan, raw, chunk_in):
    D, N = plan["delay"], raw.shape[1] // plan["down"] * plan["up"]
    dense = rt.ingest(_dev(raw))
    got, _ = _stream_all(rt, raw, chunk_in)
    assert got.shape == dense.shape == (raw.shape[0] * raw.shape[2], N) and 0 < D < N
    assert D == ref.delay(plan["up"], plan["down"], plan["width"])
    assert (_bits(got[:, :D]) == 0).all()                                                 # D leading +0
    assert torch.equal(_bits(got[:, D:]), _bits(dense[:, :N - D]))
    replay, st = _stream_all(rt, raw, chunk_in, graphs=True)
    assert st["graphs"] == 1                                                              # one captured graph served every step
    assert torch.equal(_bits(replay), _bits(got))
    return got


STREAMS = {"a": (12000, 3, 240, 12), "b": (9600, 1, 192, 12), "c": (6000, 2, 120, 12), "d": (20000, 1, 400, 12), "e": (64000, 8, 1280, 6),
           "f": (12000, 1, 6000, 3)}                                                       # case: (rate, channels, chunk_in, steps)


@pytest.mark.parametrize("case", sorted(STREAMS))
@pytest.mark.parametrize("encoding", ["int16", "ulaw"])
def test_stream_is_the_dense_output_delayed_by_D_bit_for_bit(case, encoding):
    rate, channels, chunk_in, steps = STREAMS[case]
    rt = _rt()
    plan = rt.ingest_configure(encoding, channels, rate)
    K, H = 2 * plan["width"] + plan["down"], plan["history"]
    TJ = ref.tiling(plan["up"], plan["down"], K, channels, H)
    groups = chunk_in // plan["down"]
    print(f"stream {case}: {rate} Hz {encoding} x{channels} chunk {chunk_in} ({groups} groups), H {H} D {plan['delay']} TJ {TJ} "
          f"({-(-groups // TJ)} tiles per step) {_instantiation(plan['up'])}")
    if case == "e":
        assert TJ < ref.tiling(plan["up"], plan["down"], K, 1, H) and groups > TJ       # a shrunken tile 0 beside a history, and more tiles
    if case == "f":
        assert groups >= 3 * TJ                                                          # several tiles per step
    raw = ref.random_source(encoding, (3 if channels < 8 else 2, steps * chunk_in, channels), seed=rate + chunk_in)
    _stream_equals_dense(rt, plan, raw, chunk_in)


@pytest.mark.parametrize("rate,channels", [(8000, 2), (12000, 3), (64000, 2)])
def test_one_output_group_per_step_rebuilds_the_history_from_the_history(rate, channels):
    """Case g: chunk_in = down < H, so every step's next history is mostly the old one shifted."""
    rt = _rt()
    plan = rt.ingest_configure("int16", channels, rate)
    down, H = plan["down"], plan["history"]
    steps = 3 * H // down + 4 + 3
    assert down < H and steps >= 3 * H / down + 4
    print(f"stream g: {rate} Hz x{channels} chunk {down}, H {H} D {plan['delay']}, {steps} steps {_instantiation(plan['up'])}")
    raw = ref.random_source("int16", (3, steps * down, channels), seed=rate + 1)
    _stream_equals_dense(rt, plan, raw, down)


@pytest.mark.parametrize("name,channels,chunk_in", [("a", 2, 120), ("a", 2, 30), ("d", 3, 40), ("b", 1, 64)])
def test_stream_with_a_long_history_random_table_and_its_impulses(name, channels, chunk_in):
    """Case h (table a: 63 taps over 8 phases, H = 63 input frames, D = 88 samples), beside it the longest delay in output groups
    (table d: 31) and the tap limit at up = 5 (table b): random audio against the dense call, then impulses through the stream."""
    taps, rate, up, down, width = ref.table(name)
    K = taps.shape[1]
    rt = _rt()
    plan = rt.ingest_configure("int16", channels, rate, taps=taps)
    D, H = plan["delay"], plan["history"]
    assert (D, H) == (ref.delay(up, down, width), D // up * down + width)
    if name == "a":
        assert (D // up, H) == (11, 63)
    steps = 2 * H // chunk_in + 8
    print(f"stream h: table {name} x{channels} chunk {chunk_in}, Dj {D // up} H {H} D {D}, {steps} steps {_instantiation(up)}")
    raw = ref.random_source("int16", (3, steps * chunk_in, channels), seed=rate + chunk_in)
    _stream_equals_dense(rt, plan, raw, chunk_in)
    n = steps * chunk_in
    n_out = n // down * up
    frames = [m for m in dict.fromkeys([0, 1, chunk_in - 1, chunk_in, H - 1, H, H + chunk_in, n // 2, n - H - 1, n - 1]) if 0 <= m < n]
    B = -(-len(frames) // channels) + 1
    imp = np.zeros((B, n, channels), np.int16)
    where = {}
    for i, m in enumerate(frames):
        where[i] = m
        imp[i // channels, m, i % channels] = 16384
    for graphs in (False, True):
        got, _ = _stream_all(rt, imp, chunk_in, graphs=graphs)
        _check_impulses(got.cpu().numpy(), where, taps, up, down, width, n_out, shift=D)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. UVAD_SLOT_START on the general path

@pytest.mark.parametrize("rate,channels,chunk_in", [(12000, 2, 240), (9600, 1, 192), (9600, 1, 6), (6000, 2, 3)])
def test_slot_start_on_the_general_path_restarts_one_row_and_leaves_its_neighbours_alone(rate, channels, chunk_in):
    rt = _rt()
    plan = rt.ingest_configure("int16", channels, rate)
    up, down, D = plan["up"], plan["down"], plan["delay"]
    assert up not in (1, 2)
    B, at = 3, 5
    steps = at + 4 + 2 * plan["history"] // chunk_in
    rows = B * channels
    row = rows - channels                                                                # source row 2, channel 0
    co = chunk_in // down * up
    raw = ref.random_source("int16", (B, steps * chunk_in, channels), seed=rate + chunk_in)
    plain, _ = _stream_all(rt, raw, chunk_in)
    flags = np.zeros((steps, rows), np.uint8)
    flags[at, row] = 1
    got, _ = _stream_all(rt, raw, chunk_in, flags=flags)
    others = [r for r in range(rows) if r != row]
    assert torch.equal(_bits(got[others]), _bits(plain[others]))
    assert torch.equal(_bits(got[row, :at * co]), _bits(plain[row, :at * co]))
    # a fresh stream of the remaining audio; channel 0 of a fresh multi-channel stream is what a restarted row must equal
    fresh, _ = _stream_all(rt, raw[2:3, at * chunk_in:], chunk_in)
    assert torch.equal(_bits(got[row, at * co:]), _bits(fresh[0]))
    assert (_bits(got[row, at * co:at * co + D]) == 0).all() and (got[row, at * co + D:at * co + 2 * D] != 0).any()   # the held groups, then audio
    assert not torch.equal(got[row, at * co:at * co + 2 * D], plain[row, at * co:at * co + 2 * D])
    replay, st = _stream_all(rt, raw, chunk_in, graphs=True, flags=flags)
    assert st["graphs"] == 1 and torch.equal(_bits(replay), _bits(got))
    print(f"slots: {rate} Hz x{channels} chunk {chunk_in} ({co} out), D {D} ({D // up} groups), restart at step {at}, bitwise")


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. predict_vad

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


def test_predict_vad_12k_three_channel_int16_file(tmp_path):
    from uvad_amd.scripts import predict_vad
    raw = ref.random_source("int16", (132000, 3), seed=12) // 4                          # 11 s at 12 kHz, three channels
    p = str(tmp_path / "room.wav")
    ref.write_wav(p, raw, 1, 12000)
    cfg = _predict_cfg([p], "all")
    got = {r["recording_id"]: r for r in predict_vad(**cfg)}
    assert sorted(got) == ["room.wav-ch0", "room.wav-ch1", "room.wav-ch2"]
    net, rt = _predict_model(cfg)
    rt.ingest_configure("int16", 3, 12000)
    y = rt.ingest(_dev(raw[None]))
    assert y.shape == (3, 176000)
    wins = torch.stack([y[c, w * 80000:(w + 1) * 80000] for c in range(3) for w in range(2)])   # 5 s cuts; the 1 s tail is dropped
    _, pr = rt.forward(wins, want_logits=False)
    for c in range(3):
        r = got[f"room.wav-ch{c}"]
        want = torch.cat([pr[2 * c], pr[2 * c + 1]]).cpu().numpy()
        assert r["num_frames"] == 1000 and np.array_equal(r["probs"].view(np.uint32), want[:1000].view(np.uint32)), c
