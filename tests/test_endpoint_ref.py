"""The endpointer's numpy reference (tests/endpoint_ref.py) pinned against independent statements: its labels against scipy.signal.medfilt
(a sort-based median where scipy is missing), its intervals against the buffered merge of predict.py restated here on integer frames, and
its step-wise simulator against its own whole-row answer for every cut of the frames into steps."""
import numpy as np
import pytest

import endpoint_ref as er

KERNELS = [1, 3, 5, 25, 49]
PADS = [0, 1, 7, 60]


def _median(x, K):
    """Zero-padded median of odd length K: scipy's, else by sorting every window."""
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return np.zeros(0, np.uint8)
    try:
        from scipy.signal import medfilt
        return medfilt(x, K).astype(np.uint8)
    except ImportError:
        h = K // 2
        xp = np.concatenate((np.zeros(h), x, np.zeros(h)))
        return np.array([np.sort(xp[t:t + K])[h] for t in range(len(x))]).astype(np.uint8)


def _buffered_merge(intervals, total, buffer):
    """merge_intervals_with_buffer (predict.py:614-634) on integer frames: widen, clip, sort, merge overlaps (the later end replaces)."""
    if not intervals:
        return []
    iv = sorted(([max(s - buffer, 0), min(e + buffer, total)] for s, e in intervals), key=lambda v: v[0])
    out = [list(iv[0])]
    for s, e in iv[1:]:
        if s <= out[-1][1]:
            out[-1][1] = e
        else:
            out.append([s, e])
    return [tuple(v) for v in out]


def _blocks(rng, n, around):
    """A 0/1 row of n frames in blocks whose lengths are drawn around `around`."""
    out, v = [], int(rng.integers(0, 2))
    while len(out) < n:
        out += [v] * int(max(1, around + rng.integers(-2, 3)))
        v ^= 1
    return np.array(out[:n], np.uint8)


@pytest.mark.parametrize("K", KERNELS)
def test_labels_are_the_zero_padded_median(K):
    h = K // 2
    rng = np.random.default_rng(K)
    for n in sorted({0, 1, h, h + 1, 2 * h + 1, 200}):
        for trial in range(4):
            x = (rng.random(n) < (0.3, 0.5, 0.7, 0.95)[trial]).astype(np.uint8) if trial else _blocks(rng, n, max(h, 1))
            got = er.median_labels(x, K)
            assert got.dtype == np.uint8 and got.shape == (n,)
            assert np.array_equal(got, _median(x, K)), (K, n, trial)


def test_threshold_counts_nan_and_the_threshold_itself_as_speech():
    p = np.array([0.0, 0.49999997, 0.5, 0.50000006, 1.0, np.nan, -np.inf, np.inf], np.float32)
    assert er.threshold(p, 0.5).tolist() == [0, 0, 1, 1, 1, 1, 0, 1]
    assert er.threshold(np.array([0.3, 0.29999998], np.float32), 0.3).tolist() == [1, 0]      # float32(0.3) itself is speech


@pytest.mark.parametrize("P", PADS)
def test_intervals_are_the_buffered_merge_in_frames(P):
    rng = np.random.default_rng(100 + P)
    rows = [np.zeros(0, np.uint8), np.zeros(50, np.uint8), np.ones(50, np.uint8),
            np.array([1] + [0] * 40 + [1], np.uint8),                                        # the pad reaches both clamps
            np.array(([1] * 3 + [0] * max(1, 2 * P)) * 6 + [1], np.uint8),                   # every gap is exactly 2 P: all merge
            np.array(([1] * 3 + [0] * (2 * P + 1)) * 6 + [1], np.uint8)]                     # ... one frame more: none does
    rows += [_blocks(rng, 300, a) for a in (1, 2, max(1, P), max(1, 2 * P), 2 * P + 1, 2 * P + 3)]
    for i, y in enumerate(rows):
        got = er.merged(y, P)
        assert got == _buffered_merge(er.runs(y), len(y), P), (P, i)
        if P == 0:
            assert got == er.runs(y)
        assert all(0 <= lo < hi <= len(y) for lo, hi in got)
        assert all(a[1] < b[0] for a, b in zip(got, got[1:]))
    if P:
        assert len(er.merged(rows[4], P)) == 1 and len(er.merged(rows[5], P)) == 7
    assert er.merged(rows[3], P)[0][0] == 0 and er.merged(rows[3], P)[-1][1] == 42


def test_package_restatement_agrees():
    """postprocess.merged_runs is the same rule; events_to_intervals applies the reference's rounding."""
    from uvad_amd.postprocess import events_to_intervals, merged_runs
    rng = np.random.default_rng(5)
    for P in PADS:
        for a in (1, 3, 9, 2 * P + 1):
            y = _blocks(rng, 257, a)
            assert merged_runs(y, P) == er.merged(y, P)
    assert merged_runs([], 3) == [] and merged_runs(np.ones(4), 9) == [(0, 4)]
    with pytest.raises(ValueError):
        merged_runs([1], -1)
    assert events_to_intervals([(1, 3), (2, 10), (1, 57)], 0.02) == [(0.06, 0.2), (1.14, None)]
    assert events_to_intervals(er.events_of([(0, 7), (9, 11)]), 0.01) == [(0.0, 0.07), (0.09, 0.11)]
    with pytest.raises(ValueError):
        events_to_intervals([(2, 3)], 0.02)


@pytest.mark.parametrize("K", KERNELS)
@pytest.mark.parametrize("P", PADS)
def test_simulator_is_cut_invariant_and_equals_the_whole_row(K, P):
    h, ld_in = K // 2, 8
    rng = np.random.default_rng(1000 * K + P)
    for n in (0, 1, h, h + 1, 2 * h + 1, 200):
        y_blocks = _blocks(rng, n, max(1, (h, 2 * P, 3)[n % 3]))
        p = np.where(y_blocks == 1, 0.9, 0.1).astype(np.float32)
        if n > 4:
            p[rng.integers(0, n, 3)] = np.nan
            p[rng.integers(0, n, 3)] = 0.5
        want_y, want_iv = er.whole(p, K, P)
        for cut in ("ones", "ld_in", "random"):
            sizes = []
            while sum(sizes) < n:
                sizes.append(min(n - sum(sizes), 1 if cut == "ones" else ld_in if cut == "ld_in" else int(rng.integers(0, ld_in + 1))))
            sizes.append(0)                                                  # the END step may carry no frames at all
            slot, labs, evs, pos = er.Slot(K, P), [], [], 0
            for i, k in enumerate(sizes):
                fl = (er.START if i == 0 else 0) | (er.END if i == len(sizes) - 1 else 0)
                y, ev, active = slot.step(p[pos:pos + k], fl)
                pos += k
                assert len(y) <= k + h and len(ev) <= k + h + 2
                m = pos
                if not fl & er.END:
                    assert len(np.concatenate(labs + [y])) == max(0, m - h)  # final exactly on [0, max(0, m - h))
                    open_now = len([e for e in evs + ev if e[0] == er.START]) > len([e for e in evs + ev if e[0] == er.END])
                    assert active == int(open_now)
                else:
                    assert active == 0
                labs.append(y)
                evs += ev
            assert np.array_equal(np.concatenate(labs), want_y), (K, P, n, cut)
            assert evs == er.events_of(want_iv), (K, P, n, cut)


def test_pool_helpers():
    """simulate / sessions / session_row on a small schedule: a START drops a session without events, END flushes, idle slots say nothing."""
    K, P, ld_in = 3, 1, 4
    counts = np.array([[4, 0], [4, 0], [4, 0], [2, 0]], np.int32)
    flags = np.array([[1, 0], [0, 0], [1, 0], [2, 0]], np.uint8)
    probs = np.full((4, 2, ld_in), np.nan, np.float32)
    probs[:, 0] = 0.9
    out = er.simulate(probs, counts, flags, K, P)
    assert [o[0][1] for o in out] == [[(er.START, 0)], [], [(er.START, 0)], [(er.END, 6)]]   # the first session vanished at step 2: no END(8)
    assert [o[0][2] for o in out] == [1, 1, 1, 0]
    assert all(o[1][1] == [] and o[1][2] == 0 and len(o[1][0]) == 0 for o in out)
    assert er.sessions(counts, flags) == [(0, 0, 1, False), (0, 2, 3, True), (1, 0, 3, False)]
    assert len(er.session_row(probs, counts, 0, 2, 3)) == 6
