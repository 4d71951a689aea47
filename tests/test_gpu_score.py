"""GPU tests (-m gpu) of the scoring stage (uvad_score_*, uvad_intervals_to_labels, VadRuntime.score_*, VadModel.test_step, scripts.test_vad).

  main sweep     B = 7 rows, T = 1031, ld = T + 5, lengths {1031, 257, 65, 64, 63, 1, 0}, NaN / 0xFF in the padding; segment {0, 64, 100} x
                 collar {0, 1, 3} x bins {2, 16, 1024} at the points [(0.5, 25), (0.3, 1), (0.5, 255)]: every integer output equals the
                 numpy restatement (tests/score_ref.py) exactly, the loss stays within 4 n 2^-53 relative of its float64 sum, and
                 changing the padding bytes moves nothing
  second oracle  fp / fn per row == uvad_der_counts(uvad_median_filter_lens) at threshold 0.5, collar 0, K in {1, 3, 25}
  accumulation   one step, three steps (3 + 3 + 1 rows) and reversed rows: the same integers; two identical sequences: the same loss bits
  graph          one captured score_step replayed three times with new inputs in place == three eager steps
  plus NaN, the rasteriser (byte for byte, round trip through uvad_label_runs_lens), every refusal, VadModel.test_step /
  validation_step and main(function = "test").
"""
import ctypes as C
import math
import wave

import numpy as np
import pytest
import torch

import score_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG, E_STATE = -1, -3
B, T, LD = 7, 1031, 1031 + 5
LENS = [1031, 257, 65, 64, 63, 1, 0]
POINTS = [(0.5, 25), (0.3, 1), (0.5, 255)]
SEGMENTS, COLLARS, BINS = [0, 64, 100], [0, 1, 3], [2, 16, 1024]


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def _row(rng, n):
    """n probabilities in speech / silence blocks with lengths around h = 12 and h = 127 (medians flip both ways), runs shorter than h at
    both row ends, values exactly 0, 1, 0.5 and j / 16 among them; and n reference labels with boundaries at frames 1 and n - 1."""
    p, v = [], 1
    while len(p) < n:
        k = int(max(1, (3, 12, 13, 40, 127, 128)[int(rng.integers(0, 6))] + rng.integers(-2, 3)))
        vals = rng.choice([0.9, 0.5, 1.0, 0.75, 0.3125] if v else [0.1, 0.0, 0.4375, 0.25, 0.2999], size=k)
        p += vals.tolist()
        v ^= 1
    p = np.array(p[:n], np.float32)
    p[:3] = (1.0, 0.9, 0.5)[:min(n, 3)]
    if n > 40:
        p[3:20] = 0.0
        p[-20:-2] = 0.125
        p[-2:] = 0.9375
    g = (np.cumsum(rng.random(n) < 0.03) % 2).astype(np.uint8)
    if n >= 4:
        g[0], g[1] = 1, 0
        g[n - 1] = 1 - g[n - 2]
    return p, g


def _batch(seed=11, pad_p=np.nan, pad_g=0xFF, lens=LENS):
    rng = np.random.default_rng(seed)
    p = np.full((B, LD), pad_p, np.float32)
    g = np.full((B, LD), pad_g, np.uint8)
    for b, n in enumerate(lens):
        p[b, :n], g[b, :n] = _row(rng, n)
    return p, g


_REF = {}


def _ref(collar, bins, points=tuple(POINTS)):
    key = (collar, bins, points)
    if key not in _REF:
        p, g = _batch()
        _REF[key] = sr.score(p[:, :T], g[:, :T], LENS, list(points), collar, bins)
    return _REF[key]


def _loss_ok(got, want, n):
    print(f"loss {got!r} vs {want!r}: rel {abs(got - want) / abs(want):.3e}, bound {4 * n * 2.0 ** -53:.3e}")
    return abs(got - want) <= 4 * n * 2.0 ** -53 * abs(want)


def _dev(p, g):
    return torch.from_numpy(p).to(DEV)[:, :T], torch.from_numpy(g).to(DEV)[:, :T]


def _step_and_read(rt, sc, p, g, lens=LENS, rows=True):
    r = rt.score_step(sc, p, g, lengths=lens, rows=rows)
    rows_h = r.cpu().numpy().copy() if rows else None
    return rt.score_read(sc), rows_h


@pytest.mark.parametrize("segment", SEGMENTS)
def test_main_sweep_equals_the_restatement(rt, segment):
    p, g = _batch()
    dp, dg = _dev(p, g)
    assert dp.stride(0) == LD and dg.stride(0) == LD
    p2, g2 = _batch(pad_p=0.25, pad_g=0)              # the same valid frames, other padding bytes
    dp2, dg2 = _dev(p2, g2)
    for collar in COLLARS:
        for bins in BINS:
            want = _ref(collar, bins)
            sc = rt.score_open(points=POINTS, collar=collar, bins=bins, segment=segment)
            got, rows = _step_and_read(rt, sc, dp, dg)
            tag = (segment, collar, bins)
            assert np.array_equal(got["counts"], want["counts"]), tag
            assert np.array_equal(rows, want["rows"]), tag
            assert np.array_equal(got["hist"], want["hist"]), tag
            assert got["valid"] == want["valid"] == sum(LENS) and got["steps"] == 1 and got["bins"] == bins
            assert _loss_ok(got["loss_sum"], want["loss_sum"], sum(LENS)), tag
            batch_loss = float(rt.score_batch_loss(sc).cpu())
            assert batch_loss == got["loss_sum"] / sum(LENS)
            rt.score_reset(sc)
            again, rows2 = _step_and_read(rt, sc, dp2, dg2)
            assert np.array_equal(again["counts"], got["counts"]) and np.array_equal(rows2, rows) and np.array_equal(again["hist"], got["hist"])
            assert again["loss_sum"] == got["loss_sum"], tag


def test_sweep_identity_on_the_device(rt):
    """The histogram of one pass gives the K = 1 false-alarm and miss counts of a pass at every threshold j / 16."""
    dp, dg = _dev(*_batch())
    sc = rt.score_open(points=[(0.5, 1)], collar=1, bins=16)
    hist = _step_and_read(rt, sc, dp, dg)[0]["hist"]
    for j0 in (0, 8):
        at = rt.score_open(points=[((j0 + k) / 16, 1) for k in range(8)], collar=1, bins=16)
        counts = _step_and_read(rt, at, dp, dg)[0]["counts"]
        for k in range(8):
            assert hist[0][j0 + k:].sum() == counts[k][1] and hist[1][:j0 + k].sum() == counts[k][3], j0 + k


def test_zero_probability_at_speech_is_exactly_100_per_frame(rt):
    sc = rt.score_open(points=[(0.5, 1)], bins=2)
    p = torch.zeros((2, 10), device=DEV)
    p[1] = 1.0
    g = torch.ones((2, 10), dtype=torch.uint8, device=DEV)
    g[1] = 0
    assert rt.score_read(sc)["loss_sum"] == 0.0
    rt.score_step(sc, p, g)
    assert rt.score_read(sc)["loss_sum"] == 2000.0 and float(rt.score_batch_loss(sc).cpu()) == 100.0


@pytest.mark.parametrize("kernel", [1, 3, 25])
def test_second_oracle_from_the_existing_kernels(rt, kernel):
    p, g = _batch()
    gt01 = np.zeros((B, T), np.uint8)
    for b, n in enumerate(LENS):
        gt01[b, :n] = g[b, :n]
        p[b, n:] = 0.0
    probs = torch.from_numpy(np.ascontiguousarray(p[:, :T])).to(DEV)
    pred = rt.median_filter(probs, kernel, lengths=LENS)
    der = rt.der_counts(pred, torch.from_numpy(gt01).to(DEV)).cpu().numpy()
    sc = rt.score_open(points=[(0.5, kernel)], collar=0, bins=2, segment=100)
    rows = rt.score_step(sc, probs, torch.from_numpy(gt01).to(DEV), lengths=LENS, rows=True).cpu().numpy()
    assert np.array_equal(rows[:, 1], der[:, 0]) and np.array_equal(rows[:, 3], der[:, 1])
    assert rows.sum(axis=1).tolist() == LENS


def test_accumulation_over_steps_and_row_order(rt):
    dp, dg = _dev(*_batch())
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    want = _ref(1, 16)

    def run(parts):
        sc = rt.score_open(points=POINTS, collar=1, bins=16, segment=64)
        for idx in parts:
            i = torch.tensor(idx, device=DEV)
            rt.score_step(sc, dp[i].contiguous(), dg[i].contiguous(), lengths=lens[i].contiguous())
        return rt.score_read(sc)
    one = run([list(range(B))])
    three = run([[0, 1, 2], [3, 4, 5], [6]])
    rev = run([list(range(B))[::-1]])
    for got in (one, three, rev):
        assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["hist"], want["hist"]) and got["valid"] == sum(LENS)
        assert _loss_ok(got["loss_sum"], want["loss_sum"], sum(LENS))
    assert three["steps"] == 3
    assert run([[0, 1, 2], [3, 4, 5], [6]])["loss_sum"].hex() == three["loss_sum"].hex()      # the same calls: the same bits
    assert run([list(range(B))])["loss_sum"].hex() == one["loss_sum"].hex()


def test_one_captured_graph_replays_with_new_inputs(rt):
    lens = [LENS, LENS[::-1], [5, 0, 1031, 700, 64, 2, 1]]
    batches = [_batch(seed=21 + k, lens=ln) for k, ln in enumerate(lens)]
    eager = rt.score_open(points=POINTS, collar=3, bins=16, segment=100)
    for (p, g), ln in zip(batches, lens):
        rt.score_step(eager, *_dev(p, g), lengths=ln)
    want = rt.score_read(eager)
    ref = [sr.score(p[:, :T], g[:, :T], ln, POINTS, 3, 16) for (p, g), ln in zip(batches, lens)]
    assert np.array_equal(want["counts"], sum(r["counts"] for r in ref)) and np.array_equal(want["hist"], sum(r["hist"] for r in ref))

    sc = rt.score_open(points=POINTS, collar=3, bins=16, segment=100)
    sp = torch.zeros((B, LD), device=DEV)
    sg = torch.zeros((B, LD), dtype=torch.uint8, device=DEV)
    sl = torch.zeros(B, dtype=torch.int32, device=DEV)
    rt.score_step(sc, sp[:, :T], sg[:, :T], lengths=sl, rows=True)          # sizes the workspace; nothing valid, nothing counted
    rt.score_reset(sc)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                           # one stream; a synchronisation or allocation in the step would fail here
        rows = rt.score_step(sc, sp[:, :T], sg[:, :T], lengths=sl, rows=True)
    assert rt.score_read(sc)["steps"] == 0                                   # captured, not run
    for k, ((p, g), ln) in enumerate(zip(batches, lens)):
        sp.copy_(torch.from_numpy(p).to(DEV))
        sg.copy_(torch.from_numpy(g).to(DEV))
        sl.copy_(torch.tensor(ln, dtype=torch.int32, device=DEV))
        graph.replay()
        assert np.array_equal(rows.cpu().numpy(), ref[k]["rows"])
    got = rt.score_read(sc)
    assert got["steps"] == 3 and np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["hist"], want["hist"])
    assert got["valid"] == want["valid"] and got["loss_sum"].hex() == want["loss_sum"].hex()


def test_nan_in_a_valid_frame(rt):
    p = np.full((1, 70), 0.1, np.float32)
    p[0, 33] = np.nan
    g = np.zeros((1, 70), np.uint8)
    sc = rt.score_open(points=[(0.5, 1), (0.3, 1), (0.999, 1), (0.5, 3)], bins=16, segment=64)
    got, rows = _step_and_read(rt, sc, torch.from_numpy(p).to(DEV), torch.from_numpy(g).to(DEV), lens=None)
    assert got["counts"][:3, 1].tolist() == [1, 1, 1] and got["counts"][3, 1] == 0      # speech at every threshold; one frame loses a 3-tap median
    assert got["hist"][0].tolist() == [0, 69] + [0] * 13 + [1] and rows[0].tolist() == [0, 1, 69, 0]
    assert math.isnan(got["loss_sum"]) and math.isnan(float(rt.score_batch_loss(sc).cpu()))
    want = sr.score(p, g, None, [(0.5, 1), (0.3, 1), (0.999, 1), (0.5, 3)], 0, 16)
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["hist"], want["hist"]) and math.isnan(want["loss_sum"])


def _intervals(rng, lens, max_iv):
    iv = rng.integers(-50, 1200, size=(len(lens), max_iv, 2)).astype(np.int32)      # unsorted, overlapping, reversed, out of range
    counts = np.array([4, 6, 3, 0, 5, 2, 6][:len(lens)], np.int32)
    iv[0, 0] = (900, 2000)                                                           # past the row
    iv[0, 1] = (-7, 3)                                                               # before it
    iv[0, 2] = (500, 500)                                                            # empty
    iv[0, 3] = (300, 100)                                                            # reversed
    iv[1, :6] = [(10, 20), (15, 40), (100, 130), (120, 125), (256, 258), (0, 1)]
    iv[2, :3] = [(60, 70), (0, 65), (64, 64)]
    iv[4, :5] = [(62, 63), (0, 0), (5, 1), (-3, -1), (61, 200)]
    iv[5, :2] = [(0, 1), (1, 5)]
    return iv, counts


def test_intervals_to_labels_byte_for_byte_and_round_trip(rt):
    rng = np.random.default_rng(5)
    iv, counts = _intervals(rng, LENS, 9)                                            # max_iv larger than any count
    buf = np.full((B, LD), 0xAA, np.uint8)
    want = sr.intervals_to_labels(iv, counts, T, LENS, buf)
    out = torch.from_numpy(buf).to(DEV)
    lab = rt.intervals_to_labels(iv, counts, T, lengths=LENS, out=out)
    assert np.array_equal(out.cpu().numpy(), want)                                   # bytes past each length untouched
    for b, n in enumerate(LENS):
        assert (want[b, n:] == 0xAA).all() and set(np.unique(want[b, :n])) <= {0, 1}
    assert want[0, :3].tolist() == [1, 1, 1] and want[0, 900:1031].all() and want[1, 256] == 1 and want[4, 61:63].all()
    fresh = rt.intervals_to_labels(iv, counts, T, lengths=LENS)                       # without out: zeros past the lengths
    runs, nruns = rt.label_runs(fresh.contiguous(), lengths=LENS)
    runs, nruns = runs.cpu().numpy(), nruns.cpu().numpy()
    for b, n in enumerate(LENS):
        assert np.array_equal(fresh[b, :n].cpu().numpy(), want[b, :n]) and not fresh[b, n:].any()
        d = np.diff(np.concatenate(([0], want[b, :n].astype(np.int8), [0])))
        merged = np.stack([np.flatnonzero(d == 1), np.flatnonzero(d == -1)], axis=1)
        assert nruns[b] == len(merged) and np.array_equal(runs[b, :nruns[b]], merged), b
    assert np.array_equal(lab.cpu().numpy(), want[:, :T])
    # rows longer than one workgroup's columns: intervals across the cut, no lengths
    T2 = 20000
    iv2 = np.array([[(8000, 8400), (8191, 8193), (16383, 16385), (19990, 30000)], [(0, 20000), (5, 1), (0, 0), (0, 0)]], np.int32)
    got2 = rt.intervals_to_labels(iv2, [4, 1], T2).cpu().numpy()
    assert np.array_equal(got2, sr.intervals_to_labels(iv2, [4, 1], T2, None, np.zeros((2, T2), np.uint8)))
    assert rt.intervals_to_labels(np.zeros((2, 0, 2), np.int32), [0, 0], 10).sum() == 0   # no intervals at all


def test_refusals(rt):
    from uvad_amd import _lib
    from uvad_amd.runtime import VadRuntime
    lib = rt.lib

    def cfg(points=((0.5, 25),), collar=0, bins=16, segment=64, n_points=None):
        q = _lib.ScoreCfg()
        q.n_points = len(points) if n_points is None else n_points
        for m, (t, k) in enumerate(points):
            q.threshold[m], q.kernel[m] = t, k
        q.collar, q.bins, q.segment = collar, bins, segment
        return q
    p = torch.full((2, 100), 0.7, device=DEV)
    g = torch.ones((2, 100), dtype=torch.uint8, device=DEV)
    fresh = VadRuntime(DEV)
    try:
        state = torch.zeros(1 << 15, dtype=torch.uint8, device=DEV)
        ws = torch.zeros(1 << 12, dtype=torch.uint8, device=DEV)
        step = lambda r, ld_p=100, nst=None, nws=None, st=state: lib.uvad_score_step(
            r.ctx, p.data_ptr(), ld_p, g.data_ptr(), 100, 2, 100, None, st.data_ptr(), st.numel() if nst is None else nst, None, ws.data_ptr(),
            ws.numel() if nws is None else nws, None)
        assert step(fresh) == E_STATE                                                 # not configured
        assert lib.uvad_score_reset(fresh.ctx, state.data_ptr(), state.numel(), None) == E_STATE
        for q in (cfg([(0.5, 24)]), cfg([(0.5, 257)]), cfg([(0.5, 0)]), cfg(bins=48), cfg(bins=1), cfg(bins=2048), cfg(n_points=0), cfg(n_points=9),
                  cfg(collar=-1), cfg(segment=-1)):
            assert lib.uvad_score_configure(fresh.ctx, C.byref(q)) == E_ARG
        assert lib.uvad_score_configure(fresh.ctx, C.byref(cfg())) == 0
        assert step(fresh) == E_STATE                                                 # configured, but the state was never reset
        need_s, need_w = lib.uvad_score_state_bytes(fresh.ctx), lib.uvad_score_ws_bytes(fresh.ctx, 2, 100)
        assert lib.uvad_score_reset(fresh.ctx, state.data_ptr(), need_s - 1, None) == E_ARG
        assert lib.uvad_score_reset(fresh.ctx, state.data_ptr(), need_s, None) == 0
        assert step(fresh, ld_p=99) == E_ARG and step(fresh, nst=need_s - 1) == E_ARG and step(fresh, nws=need_w - 1) == E_ARG
        assert step(fresh, nst=need_s, nws=need_w) == 0
        assert lib.uvad_score_configure(fresh.ctx, C.byref(cfg(bins=32))) == 0
        assert step(fresh) == E_STATE                                                 # reset under other bins
        assert lib.uvad_score_configure(fresh.ctx, C.byref(cfg())) == 0
        out = torch.zeros(_lib.SCORE_TOTALS_WORDS, dtype=torch.int64, device=DEV)
        assert lib.uvad_score_totals(fresh.ctx, state.data_ptr(), need_s, out.data_ptr(), None) == 0
        w = out.cpu().numpy()
        assert w[4] == 1 and w[2] == 200 and w[8:12].tolist() == [200, 0, 0, 0]         # the refused calls enqueued nothing
        lab = torch.zeros((2, 100), dtype=torch.uint8, device=DEV)
        assert lib.uvad_intervals_to_labels(fresh.ctx, None, ws.data_ptr(), 2, 1, 100, 100, None, lab.data_ptr(), None) == E_ARG
        assert lib.uvad_intervals_to_labels(fresh.ctx, ws.data_ptr(), ws.data_ptr(), 2, 1, 100, 99, None, lab.data_ptr(), None) == E_ARG
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        rt.score_open(points=[])
    with pytest.raises(ValueError):
        rt.score_open(points=[(0.5, 1)] * 9)
    with pytest.raises(Exception, match="bins"):
        rt.score_open(bins=100)
    with pytest.raises(ValueError):
        rt.score_step(rt.score_open(), p, g[:, :50])


def _vad_model():
    import uvad_amd
    from conftest import load_golden
    gold, sd, _ = load_golden("pyannet2_f80_T500")
    vm = uvad_amd.VadModel(model_name="PyanNet2", model_dict={"encoding_dim": 80})
    vm.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v for k, v in sd.items()})
    return vm.to(DEV).eval(), gold


def test_vadmodel_test_step_and_validation_step():
    from uvad_amd.postprocess import median_window, score_metrics
    vm, gold = _vad_model()
    feats = torch.from_numpy(gold["feats"]).to(DEV)
    rng = np.random.default_rng(3)
    batches = []
    for k in range(2):
        x = feats if k == 0 else torch.flip(feats, dims=[0]) * 0.5
        y = (np.cumsum(rng.random(tuple(x.shape[:2])) < 0.02, axis=1) % 2).astype(np.float32)
        batches.append({"inputs": x, "is_voice": torch.from_numpy(y)})
    with pytest.raises(RuntimeError):
        vm.test_metrics()
    for name, step, metrics, kernel in (("test", vm.test_step, vm.test_metrics, median_window(0.01)), ("val", vm.validation_step, vm.validation_metrics, 1)):
        assert kernel == (49 if name == "test" else 1)
        refs, losses = [], []
        for k, batch in enumerate(batches):
            loss = step(batch, k)
            assert torch.is_tensor(loss) and loss.is_cuda and loss.dim() == 0
            probs = vm.model(batch["inputs"]).squeeze(-1).cpu().numpy()          # the module's own probabilities
            refs.append(sr.score(probs, batch["is_voice"].numpy().astype(np.uint8), None, [(0.5, kernel)], 0, 256))
            losses.append(float(loss.cpu()))
            n = probs.size
            assert abs(losses[-1] - refs[-1]["loss_sum"] / n) <= 4 * n * 2.0 ** -53 * abs(refs[-1]["loss_sum"] / n) + 1e-300
            torch_loss = float(torch.nn.functional.binary_cross_entropy(torch.from_numpy(probs), batch["is_voice"]))
            assert abs(losses[-1] - torch_loss) < 1e-5 * abs(torch_loss)          # what the reference's _common_step returns, in f32
        pooled = {"counts": sum(r["counts"] for r in refs), "hist": sum(r["hist"] for r in refs),
                  "loss_sum": math.fsum(r["loss_sum"] for r in refs), "valid": sum(r["valid"] for r in refs)}
        want = score_metrics(pooled, prefix=name)
        got = metrics(reset=False)
        assert set(got) == set(want)
        for key in want:
            if key.endswith("_loss"):
                assert abs(got[key] - want[key]) <= 4 * pooled["valid"] * 2.0 ** -53 * abs(want[key])
            else:
                assert got[key] == want[key], key
        assert got[f"{name}_denominator"] == float(sum(b["is_voice"].numel() for b in batches))
        assert metrics(reset=True) == got
        assert metrics()[f"{name}_denominator"] == 0.0                            # reset
    with pytest.raises(NotImplementedError):
        vm.training_step({}, 0)
    with pytest.raises(NotImplementedError):
        vm.configure_optimizers()


def _write_wav(path, x):
    q = np.round(x * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(q.tobytes())


def test_main_with_function_test(tmp_path):
    import main as entry
    from config.config import load_config
    from src.scripts import predict_vad
    from uvad_amd.postprocess import det_curve, score_metrics, supervision_frames
    from uvad_amd.synth import synth_pcm
    secs = [6.2, 11.0]
    sups = [[(0.0, 1.2), (1.0, 2.503), (4.0, 7.0)], [(0.507, 3.0), (9.0, 8.0), (5.5, 10.999)]]
    paths, labels = [], []
    for k, s in enumerate(secs):
        p = tmp_path / f"r{k}.wav"
        _write_wav(p, synth_pcm(1, int(s * 16000), seed=700 + k)[0])
        f = tmp_path / f"r{k}.txt"
        f.write_text("".join(f"{a}\t{b}\tSPC\n" for a, b in sups[k]))
        paths.append(str(p)); labels.append(str(f))
    cfg = load_config()
    cfg.model_dict.encoding_dim = 64
    cfg.weights_scale = 2.0
    cfg.max_duration = 90
    cfg.input.kind = "wav"
    cfg.input.paths = paths
    cfg.input.labels = labels
    cfg.function = "test"
    got = entry.main(cfg)
    cfg.function = "predict"
    pred = predict_vad(**cfg)
    counts, hist, terms, valid, per_rec = np.zeros((1, 4), np.int64), np.zeros((2, 256), np.int64), [], 0, []
    for k, r in enumerate(pred):
        n = r["num_frames"]
        table = supervision_frames(sups[k], secs[k], frame_shift=0.01)
        gt = sr.intervals_to_labels([table], [len(table)], n, None, np.zeros((1, n), np.uint8))
        a = sr.score(r["labels"].astype(np.float32)[None], gt, None, [(0.5, 1)], 0, 2)          # predict_vad's own labels
        b = sr.score(r["probs"][None], gt, None, [(0.5, 1)], 0, 256)
        counts += a["counts"]; hist += b["hist"]; terms.append(b["loss_sum"]); valid += n
        per_rec.append((a["counts"][0][1] / n, a["counts"][0][3] / n))
    want = score_metrics({"counts": counts, "loss_sum": math.fsum(terms), "valid": valid})
    for key, v in want.items():
        if key == "test_loss":
            assert abs(got["metrics"][key] - v) <= 4 * valid * 2.0 ** -53 * abs(v)
        else:
            assert got["metrics"][key] == v, key
    assert [r["recording_id"] for r in got["recordings"]] == ["r0.wav", "r1.wav"]
    for r, (fa, md) in zip(got["recordings"], per_rec):
        assert r["false_alarm"] == fa and r["missed_detection"] == md and r["detection_error_rate"] == fa + md
    assert got["false_alarm"] == float(np.mean([fa for fa, _ in per_rec])) and got["missed_detection"] == float(np.mean([md for _, md in per_rec]))
    d = det_curve({"hist": hist})
    assert np.array_equal(got["det"]["fa_frames"], d["fa_frames"]) and got["det"]["eer"] == d["eer"] and got["det"]["best_threshold"] == d["best_threshold"]
    cfg.task = "prepare"
    with pytest.raises(NotImplementedError):
        entry.main(cfg)
