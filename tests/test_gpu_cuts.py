"""Speech cuts on the device (uvad_cuts_table, uvad_cuts_gather, include/uvad.h) against the numpy restatement tests/cuts_ref.py, byte for
byte: the cut table over a sweep of row lengths, pads and splits, the merge boundary across 64-frame words, many rows, a row several
passes long, max_cuts below the total, padding that must never be read, the gather in both types and both store forms, determinism,
one captured graph replayed with new inputs, the composition with the median filter, and predict_vad(cuts=...)."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

import cuts_ref as cr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG = -1
CANARY = 0x5A
SPAN = 4096          # frames per pass of cuts_rows_kernel (CUTS_SPAN_WORDS x 64, csrc/uvad_internal.h)


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def _table(rt, lab, T, lens, nsamp, S, cfg, max_cuts=None, expect=0):
    """One uvad_cuts_table call on lab (B, ld) uint8 with every output pre-filled with the canary and a workspace full of garbage.
    -> (code, table as CUT_DTYPE [max_cuts + 2], row_first [B + 2], total [2]) from the device."""
    from uvad_amd import _lib
    lib, ctx = rt.lib, rt.ctx
    q = _lib.CutsCfg(*cfg)
    B, ld = lab.shape
    mc = B * int(lib.uvad_cuts_max_per_row(C.byref(q), T)) if max_cuts is None else max_cuts
    d_lab = torch.from_numpy(np.ascontiguousarray(lab)).to(DEV)
    d_tab = torch.full(((mc + 2) * 32,), CANARY, dtype=torch.uint8, device=DEV)
    d_first = torch.full(((B + 2) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_total = torch.full((8,), CANARY, dtype=torch.uint8, device=DEV)
    need = max(int(lib.uvad_cuts_ws_bytes(ctx, B, T)), 16)
    ws = torch.full((need,), 0xA7, dtype=torch.uint8, device=DEV)
    d_lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    d_ns = None if nsamp is None else torch.tensor(nsamp, dtype=torch.int64, device=DEV)
    code = lib.uvad_cuts_table(ctx, d_lab.data_ptr(), ld, B, T, d_lens.data_ptr() if d_lens is not None else None,
                               d_ns.data_ptr() if d_ns is not None else None, S, C.byref(q), d_tab.data_ptr(), mc, d_first.data_ptr(),
                               d_total.data_ptr(), ws.data_ptr(), need, None)
    assert code == expect, lib.uvad_last_error(ctx)
    torch.cuda.synchronize()
    return code, d_tab.cpu().numpy().view(cr.CUT_DTYPE), d_first.cpu().numpy().view(np.int32), d_total.cpu().numpy().view(np.int32), (d_tab, d_total, mc)


def _check_table(rt, lab, T, lens, nsamp, S, cfg, max_cuts=None):
    """The call above against the restatement: total, row_first, the stored entries, and the canary in everything past them."""
    want, first = cr.table(lab[:, :T], lens, nsamp, S, cfg)
    _, tab, got_first, total, dev = _table(rt, lab, T, lens, nsamp, S, cfg, max_cuts)
    B = lab.shape[0]
    canary32 = np.frombuffer(bytes([CANARY] * 4), np.int32)[0]
    assert total[0] == len(want) and total[1] == canary32, (total, len(want))
    assert np.array_equal(got_first[:B + 1], first) and got_first[B + 1] == canary32
    kept = min(len(want), len(tab) - 2)
    assert tab[:kept].tobytes() == want[:kept].tobytes(), (cfg, lens, tab[:kept], want[:kept])
    assert set(tab[kept:].tobytes()) == {CANARY}
    return want, dev


def _mask_padding(rows, T, ld, lens):
    """rows (B, T) -> (B, ld) with every byte at or past each row's length 0xFF (a row of length 0 is 0xFF throughout)."""
    lab = np.full((rows.shape[0], ld), 0xFF, np.uint8)
    for b in range(rows.shape[0]):
        n = T if lens is None else min(max(lens[b], 0), T)
        lab[b, :n] = rows[b, :n]
    return lab


def _sweep_rows(T, seed):
    rng = np.random.default_rng(seed)
    edges = np.zeros(T, np.uint8)
    edges[:max(T // 5, 1)] = 1
    edges[T - max(T // 7, 1):] = 1
    rand = (np.cumsum(rng.random(T) < 0.15) % 2).astype(np.uint8) * np.uint8(3)     # any non-zero byte counts as 1
    return np.stack([np.zeros(T, np.uint8), np.ones(T, np.uint8), (np.arange(T) % 2).astype(np.uint8), edges, rand])


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257, 3001])
def test_table_sweep_equals_the_restatement(rt, T):
    rows = _sweep_rows(T, 100 + T)
    ld = T + 3
    cases = 0
    for P in (0, 1, 7, T + 3):
        for W, m in ((0, 0), (1, 0), (5, 2), (100, 10)):
            cfg = (P, W, m, 160, 0, 240)
            # the random row (the last) runs at lengths T, T - 1, 1 and 0; every other row kind at all four too
            for lens in (None, [T - 1] * 5, [1] * 5, [0, T, 1, T - 1, 0], [T + 9, -4, T, 1 << 30, T - 1]):
                _check_table(rt, _mask_padding(rows, T, ld, lens), T, lens, None, T * 160 + 240, cfg)
                cases += 1
    assert cases == 4 * 4 * 5


@pytest.mark.parametrize("P", [1, 5, 40])
def test_gaps_around_the_merge_bound_across_word_boundaries(rt, P):
    T = 448
    rows = []
    for g in (2 * P - 1, 2 * P, 2 * P + 1):
        for word in (64, 128, 256):
            for a in sorted({word - g - 1, word - g, word - g // 2, word - 1, word, word + 1}):   # the gap [a, a + g) around the word boundary
                if a < 3 or a + g + 3 > T:
                    continue
                row = np.zeros(T, np.uint8)
                row[a - 3:a] = 1
                row[a + g:a + g + 3] = 1
                rows.append(row)
    rows = np.stack(rows)
    assert len(rows) >= 40
    for W, m in ((0, 0), (3, 0)):
        want, _ = _check_table(rt, rows, T, None, None, T * 160, (P, W, m, 160, 0, 0))
        merged = [len(cr.merged(r, P)) for r in rows]
        assert set(merged) == {1, 2} and merged.count(1) > 10 and merged.count(2) > 5          # both sides of the boundary are in the set


def test_many_rows(rt):
    rng = np.random.default_rng(7)
    B, T = 1030, 9
    rows = (rng.random((B, T)) < 0.45).astype(np.uint8)
    lens = rng.integers(0, T + 1, B).tolist()
    want, _ = _check_table(rt, _mask_padding(rows, T, T, lens), T, lens, None, T * 160 + 240, (1, 3, 0, 160, 0, 240))
    assert len(want) > 1030 and len(set(want["row"].tolist())) > 700                 # the scan over rows runs five rounds of 256
    _check_table(rt, rows, T, None, None, T * 160 + 240, (0, 0, 0, 160, 0, 240))


def test_long_row_crosses_the_pass_span(rt):
    T = 20011
    assert T > 4 * SPAN                       # the row takes five passes of 4096 frames
    rng = np.random.default_rng(8)
    row = (np.cumsum(rng.random(T) < 0.2) % 2).astype(np.uint8)
    assert 1800 <= len(cr.runs(row)) <= 2200
    sparse = np.zeros(T, np.uint8)            # a run across a pass boundary, single frames on both sides of the next one, whole passes empty
    sparse[5:9] = 1
    sparse[SPAN - 2:SPAN + 3] = 1
    sparse[2 * SPAN - 1] = 1
    sparse[2 * SPAN + 1] = 1
    sparse[T - 3:] = 1
    full = np.ones(T, np.uint8)
    rows = np.stack([row, sparse, full])
    for cfg in ((2, 7, 1, 160, 0, 240), (0, 0, 0, 160, 0, 240), (3000, 1000, 10, 160, 0, 240), (SPAN, 0, 0, 270, 33, 721), (1, 1, 0, 160, 0, 0)):
        _check_table(rt, rows, T, None, None, T * cfg[3] + cfg[5], cfg)
    _check_table(rt, rows, T, [T - 1, 2 * SPAN + 1, SPAN], [T * 160, 123457, 0], T * 160 + 240, (2, 7, 1, 160, 0, 240))


def test_max_cuts_below_the_total(rt):
    T = 257
    rows = _sweep_rows(T, 3)
    cfg = (1, 5, 2, 160, 0, 240)
    full, _ = _check_table(rt, rows, T, None, None, T * 160 + 240, cfg)
    assert len(full) > 40
    for mc in (0, 1, 17, len(full) - 1, len(full)):
        _check_table(rt, rows, T, None, None, T * 160 + 240, cfg, max_cuts=mc)        # total and row_first stay true; the canary after the entries is intact


def _gather(rt, src, row_stride, unit, which, dev, out_rows, ld_out, offset_bytes=0):
    """One uvad_cuts_gather call into a canary-filled output of out_rows rows (and as many lengths) -> (out bytes, lengths)."""
    d_tab, d_total, mc = dev
    per = ld_out * unit
    d_out = torch.full((offset_bytes + (out_rows + 1) * per,), CANARY, dtype=torch.uint8, device=DEV)
    d_len = torch.full(((out_rows + 1) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    code = rt.lib.uvad_cuts_gather(rt.ctx, src.data_ptr(), row_stride, unit, which, d_tab.data_ptr(), d_total.data_ptr(), min(mc, out_rows),
                                   d_out.data_ptr() + offset_bytes, ld_out, d_len.data_ptr(), None)
    assert code == 0, rt.lib.uvad_last_error(rt.ctx)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[offset_bytes:], d_len.cpu().numpy().view(np.int32)


def _check_gather(rt, src_np, want_tab, dev, which, ld_out, out_rows=None, offset_bytes=0):
    """src_np (B, row_stride[, F]); everything outside the units the cuts take is poisoned (NaN / 0x7FFF) before the call."""
    key = ("first_sample", "n_samples") if which == "samples" else ("first_frame", "n_frames")
    poison = np.full_like(src_np, np.nan if src_np.dtype == np.float32 else 0x7FFF)
    for c in want_tab:
        f, n = int(c[key[0]]), min(int(c[key[1]]), ld_out)
        poison[int(c["row"]), f:f + n] = src_np[int(c["row"]), f:f + n]
    unit = src_np.dtype.itemsize * (src_np.shape[2] if src_np.ndim == 3 else 1)
    out_rows = len(want_tab) + 2 if out_rows is None else out_rows
    got, got_len = _gather(rt, torch.from_numpy(poison).to(DEV), src_np.shape[1], unit, 0 if which == "samples" else 1, dev, out_rows, ld_out,
                           offset_bytes)
    kept = min(len(want_tab), out_rows)
    shape = (out_rows + 1, ld_out) + src_np.shape[2:]
    want = np.frombuffer(bytes([CANARY]) * (int(np.prod(shape)) * src_np.dtype.itemsize), src_np.dtype).reshape(shape).copy()
    want_len = np.frombuffer(bytes([CANARY]) * ((out_rows + 1) * 4), np.int32).copy()
    cr.gather(src_np, want_tab[:kept], which, ld_out, want, want_len)                 # rows >= kept keep the canary; padding inside used rows is zero
    assert np.array_equal(got_len, want_len)
    assert got.tobytes() == want.tobytes(), (which, ld_out, src_np.dtype)


GATHER_T, GATHER_B = 300, 4


def _gather_case(rt, lead, tail):
    rng = np.random.default_rng(21)
    T, B = GATHER_T, GATHER_B
    rows = (np.cumsum(rng.random((B, T)) < 0.06, axis=1) % 2).astype(np.uint8)
    rows[0, 100:230] = 1                      # an interval of more than two full pieces
    rows[1, 280:] = 1                         # a last cut that reaches past row 1's samples
    rows[3, :] = 1
    S = T * 160 + 240
    nsamp = [S, S - 1000, 20000, 0]           # row 1: the tail clamp applies; row 2: cuts past its samples are empty; row 3: n_samples = 0 throughout
    cfg = (3, 50, 2, 160, lead, tail)
    want, dev = _check_table(rt, rows, T, None, nsamp, S, cfg)
    assert (want["n_samples"] == 0).any() and (want["n_samples"] == 50 * 160 + lead + tail).any()
    clamped = want[(want["row"] == 1)][-1]
    assert clamped["first_sample"] + clamped["n_samples"] == S - 1000
    return want, dev, S, cfg


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("lead,tail", [(0, 0), (0, 240), (33, 721)])
def test_gather_samples(rt, dtype, lead, tail):
    from uvad_amd import _lib
    want, dev, S, cfg = _gather_case(rt, lead, tail)
    rng = np.random.default_rng(5)
    stride = S + 7                                                                    # row_stride > S
    src = rng.integers(-30000, 30000, (GATHER_B, stride)).astype(np.int16) if dtype == np.int16 else rng.standard_normal((GATHER_B, stride)).astype(np.float32)
    bound = int(rt.lib.uvad_cuts_max_samples(C.byref(_lib.CutsCfg(*cfg)), S))
    assert bound == 50 * 160 + lead + tail == int(want["n_samples"].max())
    for ld_out in (bound, -(-bound // 8) * 8, bound + (1 - bound % 2) + 2, 8001 if bound > 8001 else 4001, 1):
        _check_gather(rt, src, want, dev, "samples", ld_out)
    _check_gather(rt, src, want, dev, "samples", -(-bound // 8) * 8, out_rows=5)        # fewer output rows than cuts
    _check_gather(rt, src, want, dev, "samples", -(-bound // 8) * 8, offset_bytes=4 if dtype == np.float32 else 2)   # a d_out off the 16-byte grid


@pytest.mark.parametrize("F", [1, 60, 64])
def test_gather_frames(rt, F):
    want, dev, S, cfg = _gather_case(rt, 0, 240)
    rng = np.random.default_rng(6)
    src = rng.standard_normal((GATHER_B, GATHER_T, F)).astype(np.float32)
    for ld_out in (50, 43, 53, 52, 1):
        _check_gather(rt, src, want, dev, "frames", ld_out)


def test_same_calls_same_bytes(rt):
    want, dev, S, cfg = _gather_case(rt, 33, 721)
    rng = np.random.default_rng(9)
    src = torch.from_numpy(rng.integers(-30000, 30000, (GATHER_B, S)).astype(np.int16)).to(DEV)
    rows = (np.cumsum(rng.random((GATHER_B, GATHER_T)) < 0.06, axis=1) % 2).astype(np.uint8)
    outs = []
    for _ in range(2):
        _, tab, first, total, dev = _table(rt, rows, GATHER_T, None, None, S, cfg)
        out, n = _gather(rt, src, S, 2, 0, dev, int(total[0]), 8760)
        outs.append((tab.tobytes(), first.tobytes(), total.tobytes(), out.tobytes(), n.tobytes()))
    assert outs[0] == outs[1]


def test_one_captured_graph_replays_with_new_inputs(rt):
    B, T, S = 3, 700, 700 * 160 + 240
    cfg = dict(pad=4, max_len=60, min_len=3, hop=160, lead=0, tail=240)
    rng = np.random.default_rng(31)
    batches = []
    for k in range(3):
        lab = (np.cumsum(rng.random((B, T)) < (0.02, 0.1, 0.3)[k], axis=1) % 2).astype(np.uint8)
        lens = [[T, 64, 0], [1, T - 1, 333], [650, 0, T]][k]
        nsamp = [[S, 64 * 160, 0], [400, S - 5, 333 * 160 + 240], [S, 0, 50000]][k]
        pcm = rng.integers(-30000, 30000, (B, S)).astype(np.int16)
        batches.append((lab, lens, nsamp, pcm))
    s_lab = torch.zeros((B, T), dtype=torch.uint8, device=DEV)
    s_len = torch.zeros(B, dtype=torch.int32, device=DEV)
    s_ns = torch.zeros(B, dtype=torch.int64, device=DEV)
    s_pcm = torch.zeros((B, S), dtype=torch.int16, device=DEV)
    ct = rt.cuts_open(**cfg)
    rt.speech_cuts(s_lab, s_pcm, lengths=s_len, nsamp=s_ns, cuts=ct)                    # sizes the buffers; no cut
    torch.cuda.synchronize()
    assert int(ct["total"].cpu()[0]) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                      # one stream; a synchronisation or allocation in the calls would fail here
        table, batch, lens_out = rt.speech_cuts(s_lab, s_pcm, lengths=s_len, nsamp=s_ns, cuts=ct)
    ld_out = batch.shape[1]
    assert ld_out == -(-(60 * 160 + 240) // 8) * 8
    totals = []
    for lab, lens, nsamp, pcm in batches:
        s_lab.copy_(torch.from_numpy(lab).to(DEV))
        s_len.copy_(torch.tensor(lens, dtype=torch.int32, device=DEV))
        s_ns.copy_(torch.tensor(nsamp, dtype=torch.int64, device=DEV))
        s_pcm.copy_(torch.from_numpy(pcm).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want, first = cr.table(lab, lens, nsamp, S, tuple(cfg.values()))
        n = len(want)
        totals.append(n)
        assert int(ct["total"].cpu()[0]) == n and np.array_equal(ct["row_first"].cpu().numpy(), first)
        assert rt.cuts_read(ct).tobytes() == want.tobytes()
        ref_out, ref_len = cr.gather(pcm, want, "samples", ld_out, np.zeros((n, ld_out), np.int16), np.zeros(n, np.int32))
        assert np.array_equal(batch[:n].cpu().numpy(), ref_out) and np.array_equal(lens_out[:n].cpu().numpy(), ref_len)
        e_tab, e_batch, e_len = rt.speech_cuts(torch.from_numpy(lab).to(DEV), torch.from_numpy(pcm).to(DEV), lengths=lens, nsamp=nsamp, **cfg)   # eager, fresh state
        assert torch.equal(e_tab[:n], table[:n]) and torch.equal(e_batch[:n], batch[:n]) and torch.equal(e_len[:n], lens_out[:n])
    assert min(totals) > 0 and len(set(totals)) == 3


def test_composition_with_the_median_filter(rt):
    from uvad_amd.postprocess import merged_runs
    B, T, P = 4, 1000, 10
    rng = np.random.default_rng(41)
    probs = np.clip(0.5 + 0.6 * np.sin(np.arange(T)[None, :] / rng.uniform(9, 40, (B, 1))) + 0.3 * rng.standard_normal((B, T)), 0, 1).astype(np.float32)
    lens = [T, 777, 64, 0]
    labels = rt.median_filter(torch.from_numpy(probs).to(DEV), 49, lengths=lens)        # uvad_median_filter_lens
    ct = rt.cuts_open(pad=P, max_len=0, min_len=0)
    rt.cuts_table(labels, lengths=lens, cuts=ct)
    got = rt.cuts_read(ct)
    lab = labels.cpu().numpy()
    want = [(b, lo, hi - lo) for b in range(B) for lo, hi in merged_runs(lab[b, :lens[b]], P)]
    assert len(want) >= 6
    assert [(int(c["row"]), int(c["first_frame"]), int(c["n_frames"])) for c in got] == want


def test_refusals_leave_the_outputs_untouched(rt):
    T = 100
    rows = _sweep_rows(T, 1)
    S = T * 160 + 240
    for cfg in ((-1, 0, 0, 160, 0, 240), (0, 5, 5, 160, 0, 240), (0, 0, 0, 0, 0, 240), (0, 0, 0, 160, -1, 0), (0, 0, 0, 160, 0, -1), (0, -1, 0, 160, 0, 0)):
        _, tab, first, total, _ = _table(rt, rows, T, None, None, S, cfg, max_cuts=64, expect=E_ARG)
        assert set(tab.tobytes()) | set(first.tobytes()) | set(total.tobytes()) == {CANARY}
    lib, ctx = rt.lib, rt.ctx
    from uvad_amd import _lib
    q = _lib.CutsCfg(1, 5, 2, 160, 0, 240)
    d_lab = torch.from_numpy(rows).to(DEV)
    outs = [torch.full((n,), CANARY, dtype=torch.uint8, device=DEV) for n in (64 * 32, 6 * 4, 4)]
    need = int(lib.uvad_cuts_ws_bytes(ctx, 5, T))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    call = lambda ld=T, B=5, TT=T, SS=S, mc=64, nw=need: lib.uvad_cuts_table(ctx, d_lab.data_ptr(), ld, B, TT, None, None, SS, C.byref(q), outs[0].data_ptr(), mc,
                                                                          outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), nw, None)
    for kw in ({"ld": T - 1}, {"B": 0}, {"TT": 0}, {"SS": -1}, {"mc": -1}, {"nw": need - 1}):
        assert call(**kw) == E_ARG, kw
    assert b"need" in lib.uvad_last_error(ctx)
    gout = torch.full((64 * 100 * 2,), CANARY, dtype=torch.uint8, device=DEV)
    glen = torch.full((64 * 4,), CANARY, dtype=torch.uint8, device=DEV)
    src = torch.zeros((5, S), dtype=torch.int16, device=DEV)
    g = lambda unit=2, which=0, ld_out=100, mc=64: lib.uvad_cuts_gather(ctx, src.data_ptr(), S, unit, which, outs[0].data_ptr(), outs[2].data_ptr(), mc,
                                                                        gout.data_ptr(), ld_out, glen.data_ptr(), None)
    for kw in ({"unit": 3}, {"unit": 8}, {"which": 1, "unit": 2}, {"which": 1, "unit": 4100}, {"which": 7}, {"ld_out": 0}, {"mc": -1}):
        assert g(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    for t in outs + [gout, glen]:
        assert set(t.cpu().numpy().tobytes()) == {CANARY}


def _read_wav(path):
    with wave.open(str(path), "rb") as w:
        assert w.getframerate() == 16000 and w.getnchannels() == 1 and w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), "<i2")


def _predict_with_cuts(tmp_path, frame_cfg, shift):
    """predict_vad on two synthetic 12 s recordings, without and with cuts (0.1 s buffer, split at 2 s, 0.1 s minimum, wav files written):
    frame_cfg is the integer configuration those seconds must become."""
    from config.config import load_config
    from src.scripts import predict_vad
    from uvad_amd.synth import synth_pcm
    cfg = load_config()
    if cfg.feature_extractor == "fbank":
        cfg.model_dict.encoding_dim = 64
    cfg.input.kind = "synthetic"
    cfg.input.num_utterances = 2
    cfg.input.seconds = 12.0
    cfg.input.seed = 77
    cfg.max_duration = 60
    assert cfg.cuts is None
    plain = predict_vad(**cfg)                                                         # cuts = None: what the parent commit returns
    cfg.cuts = {"buffer": 0.1, "split": True, "window": 2.0, "min": 0.1, "write_dir": str(tmp_path / "cuts")}
    got = predict_vad(**cfg)
    pcm = synth_pcm(2, int(12.0 * 16000), seed=77)
    assert [set(r) for r in plain] == [{"recording_id", "num_frames", "labels", "probs", "intervals"}] * 2
    n_cuts = 0
    for k, (g, p) in enumerate(zip(got, plain)):
        assert set(g) == set(p) | {"cuts"}
        for key in p:                                                                   # every existing output unchanged, key for key
            assert np.array_equal(g[key], p[key]) if isinstance(p[key], np.ndarray) else g[key] == p[key], key
        want, _ = cr.table(g["labels"][None, :], None, [pcm.shape[1]], pcm.shape[1], frame_cfg)
        assert [(c[2], c[3]) for c in g["cuts"]] == [(int(c["first_sample"]), int(c["n_samples"])) for c in want]
        assert [c[:2] for c in g["cuts"]] == [(round(int(c["first_frame"]) * shift, 6), round(int(c["first_frame"] + c["n_frames"]) * shift, 6)) for c in want]
        q = np.clip(np.rint(pcm[k].astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
        for i, (_, _, first, n) in enumerate(g["cuts"]):
            assert np.array_equal(_read_wav(tmp_path / "cuts" / f"{g['recording_id']}_{i:04d}.wav"), q[first:first + n])
            assert 0 < n <= frame_cfg[1] * frame_cfg[3] + frame_cfg[5]
        n_cuts += len(g["cuts"])
    print(f"predict_vad(cuts), {cfg.feature_extractor}: {n_cuts} cuts over 2 recordings")
    assert n_cuts >= 2 and len(list((tmp_path / "cuts").iterdir())) == n_cuts


def test_predict_vad_with_cuts(tmp_path):
    _predict_with_cuts(tmp_path, (10, 200, 10, 160, 0, 240), 0.01)


def test_predict_vad_with_cuts_sincnet(tmp_path, monkeypatch):
    monkeypatch.setenv("UVAD_FEATURE_EXTRACTOR", "sincnet")
    shift = 270 / 16000.0                                                              # seconds become frames by round(x / shift): 6, 119, 6
    _predict_with_cuts(tmp_path, (round(0.1 / shift), round(2.0 / shift), round(0.1 / shift), 270, 0, 721), shift)
