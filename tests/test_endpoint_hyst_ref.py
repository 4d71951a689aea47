"""The live hysteresis endpointer's step-wise simulator (tests/endpoint_hyst_ref.py) pinned without a GPU: random sessions cut at random
into steps give, concatenated, the offline restatement's intervals and labels (tests/binarize_ref.py); the header's bounds on labels and
events per step hold and the label bound is attained; the active byte takes its three values; and under onset = offset, equal pads,
min_on = 0, min_off <= 1 every step equals the median endpointer's simulator (tests/endpoint_ref.py) at kernel 1."""
import numpy as np
import pytest

import binarize_ref as br
import endpoint_hyst_ref as hr
import endpoint_ref as er

CFGS = [br.cfg(0.5), br.cfg(0.7, 0.3), br.cfg(0.7, 0.3, min_on=5), br.cfg(0.7, 0.3, min_off=6), br.cfg(0.7, 0.3, pad_on=4),
        br.cfg(0.7, 0.3, pad_off=3), br.cfg(0.7, 0.3, 3, 4, 2, 5), br.cfg(0.6, 0.6, 0, 1, 7, 0), br.cfg(0.7, 0.3, 40, 0, 9, 0),
        br.cfg(0.9, 0.1, 12, 30, 0, 6), br.cfg(0.7, 0.3, 400)]


def _blocks(rng, n, q):
    """n probabilities in HI / MID / LO blocks whose lengths are drawn around D, min_on and min_off, the thresholds themselves, the f32
    just below each and NaN among the values."""
    on, off = np.float32(q.onset), np.float32(q.offset)
    below = lambda v: np.nextafter(v, np.float32(-1))
    hi, lo = [0.95, on, np.nan], [0.02, below(off)]
    mid = [below(on), off] if off < on else []
    out = []
    while len(out) < n:
        around = (hr.gap(q), q.min_on, q.min_off, 1, 3)[int(rng.integers(0, 5))]
        k = int(max(1, around + rng.integers(-2, 3)))
        kind = int(rng.integers(0, 3 if mid else 2))
        out += rng.choice([hi, lo, mid][kind], size=k).tolist()
    return np.array(out[:n], np.float32)


def _cut(rng, n, longest=100):
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(n - sum(sizes), int(rng.integers(0, longest + 1))))
    return sizes + [0] * int(not sizes or rng.integers(0, 2))        # the END step may carry no frames at all


def _feed(q, p, sizes):
    """One session through a Slot -> per-step (labels, events, active, backlog after the step), START on the first, END on the last."""
    slot, out, pos = hr.Slot(q), [], 0
    for i, k in enumerate(sizes):
        fl = (hr.START if i == 0 else 0) | (hr.END if i == len(sizes) - 1 else 0)
        y, ev, active = slot.step(p[pos:pos + k], fl)
        pos += k
        out.append((y, ev, active, slot.backlog, k))
    return out


@pytest.mark.parametrize("qi", range(len(CFGS)))
def test_any_cut_gives_the_offline_intervals_and_labels(qi):
    q, L = CFGS[qi], hr.lag(CFGS[qi])
    rng = np.random.default_rng(50 + qi)
    seen_active, worst, kept, dropped = set(), 0, 0, 0
    for trial in range(60):
        n = int(rng.integers(0, 301)) if trial else 0
        p = _blocks(rng, n, q) if trial % 3 else rng.random(n).astype(np.float32)
        want_y, want_iv = hr.whole(p, q)
        kept += len(want_iv)
        dropped += len(br.row(p, n, q._replace(min_on=0))) - len(want_iv)
        for longest in (1, 8, 100):
            steps = _feed(q, p, _cut(rng, n, longest))
            for i, (y, ev, active, backlog, k) in enumerate(steps):
                assert len(y) <= k + L and len(ev) <= k + 1, (trial, i)
                assert 0 <= backlog <= L
                if i < len(steps) - 1:
                    worst = max(worst, backlog)
                    seen_active.add(active)
                else:
                    assert active == 0 and backlog == 0
            assert np.array_equal(np.concatenate([s[0] for s in steps]), want_y), (trial, longest)
            assert [e for s in steps for e in s[1]] == hr.events_of(want_iv), (trial, longest)
    if q.min_on > 300:
        assert kept == 0 and seen_active == {0, 2}        # longer than any session: candidates only
    elif q.min_on > q.pad_on + q.pad_off + 1:             # a one-frame run, padded, is still too short
        assert kept > 0 and dropped > 0 and seen_active == {0, 1, 2}
    else:
        assert kept > 0 and seen_active >= {0, 1} and (q.min_on > 1 or (dropped == 0 and 2 not in seen_active))
    if q.min_on == 0 and q.pad_off == 0 and q.min_off <= 1:
        assert worst == L                                 # the bound on labels per step is attained: pad_on frames owed while idle


def test_the_label_bound_is_attained_and_the_active_byte_takes_three_values():
    q = br.cfg(0.6, 0.6, 0, 1, 7, 0)                      # lag = D = pad_on = 7
    steps = _feed(q, np.full(20, 0.1, np.float32), [10, 10])
    assert hr.lag(q) == 7 and steps[0][3] == 7 and len(steps[1][0]) == 10 + 7
    q = br.cfg(0.7, 0.3, 3, 4, 2, 5)                      # D = 10, lag = 13
    p = np.array([0.1] * 5 + [0.9] + [0.5] + [0.1] * 30, np.float32)       # the run [5, 7): padded [3, 12), 9 frames, kept
    slot = hr.Slot(q)
    acts = [slot.step(p[t:t + 1])[2] for t in range(len(p))]
    assert acts[:5] == [0] * 5 and acts[5] == 1           # lo = 3: with the frame itself the interval already has 3 frames
    q = br.cfg(0.7, 0.3, 6, 0, 0, 0)
    slot = hr.Slot(q)
    acts = [slot.step(np.float32([v]))[2] for v in [0.1, 0.9, 0.5, 0.5, 0.1, 0.9, 0.9, 0.5, 0.5, 0.5, 0.5, 0.1]]
    assert acts == [0, 2, 2, 2, 0, 2, 2, 2, 2, 2, 1, 0]  # a candidate dropped, one confirmed by its sixth frame


@pytest.mark.parametrize("P", [0, 1, 7])
@pytest.mark.parametrize("min_off", [0, 1])
@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_reduction_to_the_median_endpointer_at_kernel_1(P, min_off, thr):
    q = br.cfg(thr, thr, 0, min_off, P, P)
    rng = np.random.default_rng(7 + P)
    for trial in range(10):
        n = int(rng.integers(0, 301))
        p = _blocks(rng, n, q)
        a, b, pos = hr.Slot(q), er.Slot(1, P, thr), 0
        sizes = _cut(rng, n, 8)
        for i, k in enumerate(sizes):
            fl = (hr.START if i == 0 else 0) | (hr.END if i == len(sizes) - 1 else 0)
            _, ev, active = a.step(p[pos:pos + k], fl)
            _, ev2, active2 = b.step(p[pos:pos + k], fl)
            pos += k
            assert ev == ev2 and active == active2, (trial, i)


def test_pool_helper_and_flags():
    """simulate on a small schedule: a START drops a session without events, END flushes an unconfirmed candidate without events."""
    q = br.cfg(0.7, 0.3, min_on=6)
    counts = np.array([[4, 0], [4, 0], [4, 0], [1, 0]], np.int32)
    flags = np.array([[1, 0], [0, 0], [1, 0], [2, 0]], np.uint8)
    probs = np.full((4, 2, 4), np.nan, np.float32)
    probs[:, 0] = 0.9
    out = hr.simulate(probs, counts, flags, q)
    assert [o[0][1] for o in out] == [[], [(hr.START, 0)], [], []]            # 8 frames confirmed, then dropped by START; 5 frames: never confirmed
    assert [o[0][2] for o in out] == [2, 1, 2, 0]
    assert [len(o[0][0]) for o in out] == [0, 8, 0, 5] and not out[3][0][0].any()
    assert all(o[1][1] == [] and o[1][2] == 0 and len(o[1][0]) == 0 for o in out)
