"""Hysteresis decisions on the device (uvad_binarize, include/uvad.h) against the frame-loop restatement tests/binarize_ref.py, byte for
byte: a sweep of row lengths, layouts and configurations, the state carried across words, segments and passes, the fill and drop
boundaries at those seams, max_iv below the count, the composition with the neighbouring entry points, determinism, one captured graph
replayed with new inputs, the runtime's calls and predict_vad(binarize=...) in its three routes."""
import ctypes as C

import numpy as np
import pytest
import torch

import binarize_ref as br

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG = -1
CANARY = 0x5A
CANARY32 = int(np.frombuffer(bytes([CANARY] * 4), np.int32)[0])
SPAN = 4096          # frames per pass of binarize_rows_kernel (BIN_SPAN_WORDS x 64, csrc/uvad_internal.h)
SEG = 2048           # frames per workgroup of binarize_classify_kernel (BIN_SEG)
H, M, L = 0.9, 0.5, 0.1
HYST = dict(onset=0.7, offset=0.3)


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def _pad_nan(rows, ld_p, lens):
    """rows (B, T) -> (B, ld_p) with every value at or past each row's length NaN (which would count as speech if it were read)."""
    B, T = rows.shape
    p = np.full((B, ld_p), np.nan, np.float32)
    for b in range(B):
        n = T if lens is None else min(max(lens[b], 0), T)
        p[b, :n] = rows[b, :n]
    return p


def _call(rt, rows, lens, q, max_iv=None, labels=True, ld_p=None, expect=0):
    """One uvad_binarize call on rows (B, T): the probabilities laid out with stride ld_p and NaN in the padding, every output pre-filled
    with the canary, the workspace full of garbage.  -> (labels (B, T + 5) or None, iv (B x max_iv + 2, 2), counts (B + 1,)) from the device."""
    from uvad_amd import _lib
    lib, ctx = rt.lib, rt.ctx
    B, T = rows.shape
    ld_p = T if ld_p is None else ld_p
    mi = (T + 1) // 2 if max_iv is None else max_iv
    d_p = torch.from_numpy(_pad_nan(rows, ld_p, lens)).to(DEV)
    d_lab = torch.full((B, T + 5), CANARY, dtype=torch.uint8, device=DEV) if labels else None
    d_iv = torch.full((B * mi + 2, 2), CANARY32, dtype=torch.int32, device=DEV)
    d_cn = torch.full((B + 1,), CANARY32, dtype=torch.int32, device=DEV)
    need = max(int(lib.uvad_binarize_ws_bytes(ctx, B, T)), 16)
    ws = torch.full((need,), 0xA7, dtype=torch.uint8, device=DEV)
    d_lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    cfg = _lib.BinarizeCfg(*q)
    code = lib.uvad_binarize(ctx, d_p.data_ptr(), ld_p, B, T, d_lens.data_ptr() if d_lens is not None else None, C.byref(cfg),
                             d_lab.data_ptr() if labels else None, T + 5, d_iv.data_ptr() if mi else None, mi, d_cn.data_ptr(),
                             ws.data_ptr(), need, None)
    assert code == expect, lib.uvad_last_error(ctx)
    torch.cuda.synchronize()
    return d_lab.cpu().numpy() if labels else None, d_iv.cpu().numpy(), d_cn.cpu().numpy()


def _check(rt, rows, lens, q, max_iv=None, labels=True, ld_p=None):
    """The call above against the restatement, byte for byte: bytes the call must not write (past the counts, past each row's length, past
    the arrays' used part) keep the canary on both sides.  -> the per-row interval lists."""
    B, T = rows.shape
    mi = (T + 1) // 2 if max_iv is None else max_iv
    lab, iv, cn = _call(rt, rows, lens, q, max_iv, labels, ld_p)
    want_lab, want_iv, want_cn = br.outputs(rows, lens, q, mi, np.full((B, T + 5), CANARY, np.uint8) if labels else None,
                                            np.full((B, mi, 2), CANARY32, np.int32), np.full(B, CANARY32, np.int32))
    assert np.array_equal(cn[:B], want_cn) and cn[B] == CANARY32, (q, lens, cn, want_cn)
    assert iv[:B * mi].tobytes() == want_iv.tobytes(), (q, lens)
    assert (iv[B * mi:] == CANARY32).all()
    if labels:
        assert lab.tobytes() == want_lab.tobytes(), (q, lens)
    return br.batch(rows, lens, q)


def _stretches(rng, T, longest):
    """T probabilities in HI, LO and MID stretches of random length, some exactly at the two thresholds of HYST, a few NaN."""
    p, t = np.empty(T, np.float32), 0
    while t < T:
        n = int(rng.integers(1, int(rng.choice([2, 5, longest])) + 1))
        kind = int(rng.integers(0, 5))
        p[t:t + n] = (H, M, L, 0.7, 0.3)[kind] + (rng.uniform(-0.05, 0.05) if kind < 3 else 0.0)
        t += n
    if T > 10:
        p[rng.integers(0, T, 2)] = np.nan
    return p


def _ld_pair(T):
    """Two row strides > T: a multiple of four floats (every row 16-byte aligned: the 16-byte loads) and not one (the 4-byte loads)."""
    ld = (T + 4) // 4 * 4
    return ld, ld + 1


@pytest.mark.parametrize("T", [1, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 37])
def test_sweep_equals_the_restatement(rt, T):
    rng = np.random.default_rng(100 + T)
    B = 6
    rows = np.stack([_stretches(rng, T, (3, 40, 200, 700, 64, 9)[b]) for b in range(B)])
    rows[4, :] = M if T > 1 else H                                 # all MID: nothing ever turns on
    if T > 2:
        rows[4, T // 3] = H                                        # ... but for one frame: on to the row's end
    lens_list = (None, [0, 1, T, int(rng.integers(0, T + 1)), int(rng.integers(0, T + 1)), T - 1], [T + 9, -4, T, 1 << 30, T // 2, 0])
    cfgs = [br.cfg(0.5), br.cfg(**HYST), br.cfg(**HYST, min_on=3, min_off=2, pad_on=1, pad_off=2), br.cfg(**HYST, min_on=T + 1),
            br.cfg(0.6, 0.6, min_on=5, min_off=9, pad_off=4), br.cfg(0.8, 0.2, min_off=70, pad_on=65, pad_off=3)]
    kept = 0
    for k, q in enumerate(cfgs):
        for j, lens in enumerate(lens_list):
            got = _check(rt, rows, lens, q, ld_p=_ld_pair(T)[(k + j) % 2])
            kept += sum(len(r) for r in got)
            if q.min_on > T:
                assert all(r == [] for r in got)
    _check(rt, rows[:1], None, cfgs[2], ld_p=T)                    # one row: its stride does not matter
    _check(rt, rows, None, cfgs[2], labels=False, ld_p=T)          # without labels
    assert kept > 0


def test_state_carried_across_words_segments_and_passes(rt):
    T = 2 * SPAN + 40
    ks = [63, 64, 65, SEG - 1, SEG + 1, SPAN - 1, SPAN + 1, 2 * SPAN + 1]
    rows = []
    for k in ks:
        for a in (0, 5):
            on = np.full(T, M, np.float32)                         # one HI frame, MID up to k, one LO frame, MID again
            on[:a] = L
            on[a] = H
            on[k] = L
            off = on.copy()                                        # the same without the HI frame: the state stays 0 throughout
            off[a] = M
            rows += [on, off]
    rows = np.stack(rows)
    for ld_p in _ld_pair(T):
        got = _check(rt, rows, None, br.cfg(**HYST), ld_p=ld_p)
        assert got == [r for k in ks for a in (0, 5) for r in ([(a, k)], [])]
    got = _check(rt, rows, [k for k in ks for _ in range(4)], br.cfg(**HYST))          # the row ends where the LO frame stood
    assert got == [r for k in ks for a in (0, 5) for r in ([(a, k)], [])]


@pytest.mark.parametrize("pads", [(0, 0, 0), (0, 0, 1), (0, 0, 2), (3, 0, 0), (0, 5, 0), (2, 3, 7)])
def test_fill_boundary_across_word_segment_and_pass(rt, pads):
    pad_on, pad_off, min_off = pads
    D = pad_on + pad_off + max(min_off - 1, 0)
    T = SPAN + 200
    rows, merged = [], []
    for gap in (D, D + 1):
        for seam in (64, SEG, SPAN):
            for c in sorted({seam - gap, seam - gap // 2, seam, seam - 1}):   # the pause [c, c + gap) around the seam
                row = np.full(T, L, np.float32)
                row[c - 1] = H
                row[c + gap] = H
                rows.append(row)
                merged.append(gap <= D)
    rows = np.stack(rows)
    q = br.cfg(**HYST, min_off=min_off, pad_on=pad_on, pad_off=pad_off)
    for ld_p in _ld_pair(T):
        got = _check(rt, rows, None, q, ld_p=ld_p)
        assert [len(r) == 1 for r in got] == merged and {len(r) for r in got} == {1, 2}


def test_drop_boundary_at_the_row_ends_and_across_a_pass(rt):
    T, m = SPAN + 300, 10
    q = br.cfg(**HYST, min_on=m, pad_on=3, pad_off=2)
    rows, lens = [], []
    for extra in (0, 1):                                           # m - 1 frames, then m frames, after padding and clipping
        for where in ("start", "end", "pass", "clipped"):
            row = np.full(T, L, np.float32)
            n = T
            if where == "start":                                   # [1, 1 + r) -> [0, r + 3)
                row[1:1 + m - 4 + extra] = H
            elif where == "end":                                   # [T - 1 - r, T - 1) -> [T - 4 - r, T)
                row[T - 1 - (m - 5 + extra):T - 1] = H
            elif where == "pass":                                  # [SPAN - 4, SPAN - 4 + r) -> [SPAN - 7, SPAN - 2 + r), closed by a later start
                row[SPAN - 4:SPAN - 4 + m - 6 + extra] = H
                row[SPAN + 150:SPAN + 200] = H
            else:                                                  # as "end", with the row's end given by its length
                n = SPAN + 100
                row[n - 1 - (m - 5 + extra):n - 1] = H
                row[n:] = H
            rows.append(row)
            lens.append(n)
    got = _check(rt, np.stack(rows), lens, q)
    assert [len(r) for r in got] == [0, 0, 1, 0, 1, 1, 2, 1]
    assert [r[0][1] - r[0][0] for r in got[4:]] == [m] * 4 and got[2] == [(SPAN + 147, SPAN + 202)]


def test_long_minimum_duration(rt):
    T, m = 70000, 66000
    rows = np.full((2, T), M, np.float32)
    rows[:, :100] = L
    rows[:, 100] = H
    rows[0, 100 + m - 1] = L                                       # 65 999 frames
    rows[1, 100 + m] = L                                           # 66 000 frames
    got = _check(rt, rows, None, br.cfg(**HYST, min_on=m), max_iv=4)
    assert got == [[], [(100, 100 + m)]]


def test_max_iv_below_the_count(rt):
    rng = np.random.default_rng(5)
    T = 700
    rows = np.stack([_stretches(rng, T, 9) for _ in range(3)])
    q = br.cfg(**HYST, min_off=2)
    full = _check(rt, rows, None, q)
    most, least = max(len(r) for r in full), min(len(r) for r in full)
    assert least > 20
    for mi in (0, 1, least - 1, least, most - 1, most):            # the counts stay true, the labels complete, the canary after the entries intact
        _check(rt, rows, [T, T - 1, 600], q, max_iv=mi)


def test_composition_with_the_neighbouring_entry_points(rt):
    rng = np.random.default_rng(6)
    B, T = 4, 1500
    rows = np.stack([_stretches(rng, T, 30) for _ in range(B)])
    rows[~np.isfinite(rows)] = H
    lens = [T, 777, 64, 0]
    probs = torch.from_numpy(rows).to(DEV)
    st = rt.binarize_open(**HYST, min_on=4, min_off=6, pad_on=2, pad_off=3)
    lab, iv, cn = rt.binarize(probs, lengths=lens, state=st)
    assert int(cn.sum()) > 20
    again = rt.intervals_to_labels(iv, cn, T, lengths=lens)                             # uvad_intervals_to_labels on (d_iv, d_iv_counts)
    assert torch.equal(again, lab)
    ct = rt.cuts_open(pad=0, max_len=0, min_len=0)                                     # uvad_cuts_table with pad 0 lists exactly the intervals
    rt.cuts_table(lab, lengths=lens, cuts=ct)
    want = [(b, lo, hi - lo) for b, r in enumerate(rt.binarize_read(st)) for lo, hi in r]
    assert [(int(c["row"]), int(c["first_frame"]), int(c["n_frames"])) for c in rt.cuts_read(ct)] == want
    lab0, _, _ = rt.binarize(probs, lengths=lens, onset=0.5)                            # one threshold, no durations: the raw threshold's labels
    med = rt.median_filter(probs, 1, lengths=lens)                                     # uvad_median_filter_lens, kernel = 1
    for b in range(B):
        assert torch.equal(lab0[b, :lens[b]], med[b, :lens[b]].to(torch.uint8))


def test_same_calls_same_bytes(rt):
    rng = np.random.default_rng(7)
    T = SPAN + 77
    rows = np.stack([_stretches(rng, T, 50) for _ in range(5)])
    q = br.cfg(**HYST, min_on=3, min_off=4, pad_on=1, pad_off=1)
    outs = [tuple(a.tobytes() for a in _call(rt, rows, [T, 5, 4000, SPAN, 0], q, ld_p=T + 3)) for _ in range(2)]
    assert outs[0] == outs[1]


def test_one_captured_graph_replays_with_new_inputs(rt):
    B, T = 3, SPAN + 500
    kw = dict(**HYST, min_on=5, min_off=8, pad_on=2, pad_off=4)
    q = br.cfg(**kw)
    rng = np.random.default_rng(31)
    batches = [(np.stack([_stretches(rng, T, (200, 30, 8)[k]) for _ in range(B)]), [[T, 64, 0], [1, T - 1, 333], [SPAN, 0, T]][k]) for k in range(3)]
    s_p = torch.full((B, T), L, dtype=torch.float32, device=DEV)
    s_len = torch.zeros(B, dtype=torch.int32, device=DEV)
    st = rt.binarize_open(**kw)
    rt.binarize(s_p, lengths=s_len, state=st)                                          # sizes the buffers; no interval
    torch.cuda.synchronize()
    assert int(st["counts"].sum()) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                      # one stream; a synchronisation or allocation in the call would fail here
        lab, iv, cn = rt.binarize(s_p, lengths=s_len, state=st)
    totals = []
    for rows, lens in batches:
        s_p.copy_(torch.from_numpy(rows).to(DEV))
        s_len.copy_(torch.tensor(lens, dtype=torch.int32, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = br.batch(rows, lens, q)
        assert rt.binarize_read(st) == want
        for b in range(B):
            assert np.array_equal(lab[b, :lens[b]].cpu().numpy(), br.labels_of(want[b], lens[b]))
        e_lab, e_iv, e_cn = rt.binarize(torch.from_numpy(rows).to(DEV), lengths=lens, **kw)   # eager, fresh state
        assert torch.equal(e_cn, cn)
        for b in range(B):
            assert torch.equal(e_iv[b, :int(cn[b])], iv[b, :int(cn[b])]) and torch.equal(e_lab[b, :lens[b]], lab[b, :lens[b]])
        totals.append(sum(len(r) for r in want))
    assert min(totals) > 0 and len(set(totals)) == 3


def test_refusals_leave_the_outputs_untouched(rt):
    rows = np.full((3, 100), H, np.float32)
    for q in ((0.3, 0.5, 0, 0, 0, 0), (float("nan"), 0.5, 0, 0, 0, 0), (0.5, 0.5, -1, 0, 0, 0), (0.5, 0.5, 0, (1 << 20) + 1, 0, 0),
              (0.5, 0.5, 0, 0, -1, 0), (0.5, 0.5, 0, 0, 0, -7)):
        lab, iv, cn = _call(rt, rows, None, q, expect=E_ARG)
        assert set(lab.tobytes()) | set(iv.tobytes()) | set(cn.tobytes()) == {CANARY}


def test_runtime_calls(rt):
    rows = np.full((3, 40), L, np.float32)
    rows[0, 3:9] = H
    rows[0, 9:14] = M
    rows[1, 20] = H
    rows[2, 0:2] = H
    rows[2, 5:40] = H
    probs = torch.from_numpy(rows).to(DEV)
    st = rt.binarize_open(**HYST, min_on=2, pad_off=1)
    lab, iv, cn = rt.binarize(probs, lengths=[40, 40, 30], state=st)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (3, 40) and tuple(iv.shape) == (3, 20, 2) and iv.dtype == cn.dtype == torch.int32
    assert rt.binarize_read(st) == [[(3, 15)], [(20, 22)], [(0, 3), (5, 30)]] == br.batch(rows, [40, 40, 30], br.cfg(**HYST, min_on=2, pad_off=1))
    assert cn.tolist() == [1, 1, 2] and lab[2].tolist() == [1] * 3 + [0] * 2 + [1] * 25 + [0] * 10
    none, iv1, cn1 = rt.binarize(probs[:, :30], labels=False, max_iv=1, **HYST)       # a row-strided view, no labels, one interval stored
    assert none is None and tuple(iv1.shape) == (3, 1, 2) and cn1.tolist() == [1, 1, 2] and iv1[:, 0].tolist() == [[3, 14], [20, 21], [0, 2]]
    for bad in (dict(onset=0.3, offset=0.5), dict(onset=float("inf")), dict(min_on=-1), dict(pad_off=(1 << 20) + 1), dict(min_off=1.5), dict(max_iv=-1)):
        with pytest.raises(ValueError, match="2\\^20|max_iv"):
            rt.binarize_open(**bad)
    with pytest.raises(ValueError):
        rt.binarize(probs.double())


def _predict(route, sincnet):
    """predict_vad on two synthetic 12 s recordings, without and with binarize, in one route -> (plain, got, cfg)."""
    from config.config import load_config
    from src.scripts import predict_vad
    cfg = load_config()
    if cfg.feature_extractor == "fbank":
        cfg.model_dict.encoding_dim = 64
    assert (cfg.feature_extractor == "sincnet") == sincnet
    cfg.input.kind = "synthetic"
    cfg.input.num_utterances = 2
    cfg.input.seconds = 12.0
    cfg.input.seed = 77
    cfg.max_duration = 60
    if route == "ragged":
        cfg.window_seconds = None
        cfg.ragged_batches = True
    elif route == "sliding":
        cfg.hop_seconds = 2.5
    assert cfg.binarize is None
    plain = predict_vad(**cfg)                                                         # binarize = None: the median path
    cfg.binarize = {"onset": 0.55, "offset": 0.45, "min_duration_on": 0.05, "min_duration_off": 0.08, "pad_onset": 0.02, "pad_offset": 0.03}
    return plain, predict_vad(**cfg), cfg


def _check_predict(rt, route, sincnet):
    from uvad_amd.postprocess import labels_to_intervals_batch, median_window, sincnet_frame_times, sincnet_labels_to_intervals
    plain, got, cfg = _predict(route, sincnet)
    shift = 270 / 16000.0 if sincnet else 0.01
    fr = lambda s: int(round(s / shift))
    q = br.cfg(0.55, 0.45, fr(0.05), fr(0.08), fr(0.02), fr(0.03))
    speech = frames = 0
    for g, p in zip(got, plain):
        assert set(g) == set(p) == {"recording_id", "num_frames", "labels", "probs", "intervals"}
        assert g["num_frames"] == p["num_frames"] == len(g["labels"]) and np.array_equal(g["probs"], p["probs"]) and g["labels"].dtype == np.uint8
        n = g["num_frames"]
        want = br.row(g["probs"], n, q)                                                 # the restatement on the probabilities the call returned
        assert np.array_equal(g["labels"], br.labels_of(want, n))
        secs = [sincnet_frame_times(lo, hi - 1, 12.0) if sincnet else (round(lo * 0.01, 2), round((hi - 1) * 0.01, 2)) for lo, hi in want]
        assert g["intervals"] == [(s, e) for s, e in secs if e - s > 0]
        # without the option: the median path's own kernels on the same probabilities, row by row as the route lays them out
        per = (293 if sincnet else 500) if route == "disjoint" else n                  # disjoint: every window's frames are kept whole here
        assert n and n % per == 0
        lab = rt.median_filter(torch.from_numpy(p["probs"]).to(DEV).reshape(-1, per), median_window(0.01)).reshape(-1)
        assert np.array_equal(p["labels"], lab.cpu().numpy().astype(np.uint8))
        ivs = sincnet_labels_to_intervals(lab, 12.0, runtime=rt) if sincnet else labels_to_intervals_batch(lab.reshape(1, -1), 0.01, runtime=rt)[0]
        assert p["intervals"] == ivs
        speech += int(g["labels"].sum())
        frames += n
    print(f"predict_vad(binarize), {route}, {'sincnet' if sincnet else 'fbank'}: {speech} speech frames of {frames}")
    assert 0 < speech < frames


@pytest.mark.parametrize("route", ["disjoint", "ragged", "sliding"])
def test_predict_vad_with_binarize(rt, route):
    _check_predict(rt, route, False)


def test_predict_vad_with_binarize_sincnet(rt, monkeypatch):
    monkeypatch.setenv("UVAD_FEATURE_EXTRACTOR", "sincnet")
    _check_predict(rt, "disjoint", True)
