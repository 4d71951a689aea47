"""The numpy restatement of the speech cuts (tests/cuts_ref.py) against three other statements of the same thing: the package's host
functions, the project's float-seconds merge and split fed integer frames, and a frame-by-frame walk; and the closed form of the split
against the reference's loop."""
import numpy as np
import pytest

import cuts_ref as cr

CASES = [(0, 0, 0), (0, 1, 0), (1, 5, 2), (7, 100, 10), (3, 0, 4), (40, 64, 63), (2, 3, 0)]


def _rows(seed, count=60):
    rng = np.random.default_rng(seed)
    rows = [np.zeros(0, np.uint8), np.zeros(9, np.uint8), np.ones(1, np.uint8), np.ones(130, np.uint8), (np.arange(67) % 2).astype(np.uint8)]
    for _ in range(count):
        n = int(rng.integers(1, 400))
        p = float(rng.choice([0.03, 0.2, 0.5, 0.9]))
        flips = rng.random(n) < p * 0.3
        row = (np.cumsum(flips) % 2).astype(np.uint8) if rng.random() < 0.5 else (rng.random(n) < p).astype(np.uint8)
        rows.append(row * np.uint8(rng.choice([1, 255])))
    return rows


@pytest.mark.parametrize("pad,max_len,min_len", CASES)
def test_restatement_equals_the_host_functions(pad, max_len, min_len):
    from uvad_amd.postprocess import cut_table, merged_runs, split_runs
    for row in _rows(1):
        want = [(f, f + k) for f, k in cr.row_cuts(row, pad, max_len, min_len)]
        assert cut_table(row != 0, pad, max_len, min_len) == want
        assert split_runs(merged_runs(row != 0, pad), max_len, min_len) == want
        assert cr.merged(row, pad) == merged_runs(row != 0, pad)


def _split_with_threshold(intervals, window, keep_above):
    # split_into_windows of src/scripts/predict.py:638-647, restated with its literal 0.1 made the parameter keep_above
    out = []
    for s, e in intervals:
        while e - s > window:
            out.append([s, s + window])
            s += window
        if e - s > keep_above:
            out.append([s, e])
    return out


@pytest.mark.parametrize("pad,max_len,min_len", [c for c in CASES if c[1] > 0])
def test_restatement_equals_the_float_functions_on_integer_frames(pad, max_len, min_len):
    from uvad_amd.postprocess import merge_intervals_with_buffer, split_into_windows
    for row in _rows(2):
        runs = cr.runs(row)
        merged = merge_intervals_with_buffer([(float(s), float(c)) for s, c in runs], float(len(row)), float(pad))
        assert [(int(a), int(b)) for a, b in merged] == cr.merged(row, pad)
        want = [(int(s), int(e - s)) for s, e in _split_with_threshold(merged, float(max_len), float(min_len))]
        assert cr.row_cuts(row, pad, max_len, min_len) == want
        if min_len == 0:   # the project's own function as it stands: its 0.1 drops nothing an integer m = 0 keeps
            assert [(int(s), int(e - s)) for s, e in split_into_windows(merged, float(max_len))] == want


@pytest.mark.parametrize("pad,max_len,min_len", CASES)
def test_restatement_equals_a_frame_by_frame_walk(pad, max_len, min_len):
    for row in _rows(3, 40):
        n = len(row)
        covered = np.zeros(n, bool)                       # frames inside some widened run
        for t in range(n):
            if row[t]:
                covered[max(t - pad, 0):min(t + pad + 1, n)] = True
        # widened runs that only touch (start == predecessor's end) merge too: a gap of exactly 2 pad frames leaves no uncovered frame
        # between them, so the union's components are the merged intervals
        pieces, t = [], 0
        while t < n:
            if not covered[t]:
                t += 1
                continue
            e = t
            while e < n and covered[e]:
                e += 1
            s = t
            while max_len and e - s > max_len:
                pieces.append((s, max_len))
                s += max_len
            if e - s > min_len:
                pieces.append((s, e - s))
            t = e
        assert cr.row_cuts(row, pad, max_len, min_len) == pieces


@pytest.mark.parametrize("W,m", [(1, 0), (2, 0), (2, 1), (5, 2), (7, 6), (100, 10)])
def test_closed_form_of_the_split(W, m):
    for L in range(1, 3 * W + 2):
        q, r = (L - 1) // W, L - ((L - 1) // W) * W
        assert 0 < r <= W
        loop = cr.split([(11, 11 + L)], W, m)
        want = [(11 + j * W, 11 + (j + 1) * W) for j in range(q)] + ([(11 + q * W, 11 + L)] if r > m else [])
        assert loop == want


def test_table_and_gather_of_the_restatement():
    lab = np.zeros((3, 20), np.uint8)
    lab[0, 2:5] = 1
    lab[0, 9:20] = 1
    lab[2, 0:20] = 7
    tab, first = cr.table(lab, [20, 20, 13], [3000, 0, 1000], 3000, (1, 6, 1, 160, 33, 240))
    assert first.tolist() == [0, 3, 3, 5]
    assert [tuple(int(v) for v in c) for c in tab] == [
        (0, 0, 1, 5, 127, 1073), (0, 1, 8, 6, 1247, 1233), (0, 2, 14, 6, 2207, 793),      # the last one clipped at S_b = 3000
        (2, 0, 0, 6, 0, 1000), (2, 1, 6, 6, 927, 73)]                                     # 13 frames: 6 + 6, the last 1 <= m dropped
    src = np.arange(3 * 3000, dtype=np.int16).reshape(3, 3000)
    out, n = cr.gather(src, tab, "samples", 1100, np.full((len(tab), 1100), -1, np.int16), np.full(len(tab), -1, np.int32))
    assert n.tolist() == [min(int(c["n_samples"]), 1100) for c in tab]
    assert out[0, :1073].tolist() == src[0, 127:1200].tolist() and not out[0, 1073:].any()
