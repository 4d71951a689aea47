"""GPU tests (-m gpu) of the live hysteresis endpointer (uvad_endpoint_hyst_*, VadRuntime.endpoint_hyst_*): B = 5 slots, ld_in = 8, 60 steps
of 0 .. 8 frames per slot, under the configurations CFGS.

  step-wise   every step's events, counts, active byte, labels and label counts equal the frame-loop simulator (tests/endpoint_hyst_ref.py)
  offline     every ended session equals uvad_binarize run on the device over the session's whole row: interval list and label bytes
  cuts        the same sessions fed 1 frame or a random number of frames at a time give the same labels and events
  isolation   0.0 or +Inf instead of NaN in columns >= n_b and in rows with n_b = 0 change no output byte
  overflow    max_events = 1 counts truly, keeps the first event and harms no state
  one graph   a graph captured around step 3 replays every later step to the eager run's bytes
  reduction   onset = offset, equal pads, min_on = 0, min_off <= 1: every step's events and active byte are uvad_endpoint_step's at kernel 1
  plus ld_in = 130 (three ballot words, the last partial), min_on = 300 with pad_on = 40 against steps of 3 frames, and every refusal
  (state and outputs untouched).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import binarize_ref as br
import endpoint_hyst_ref as hr
import endpoint_ref as er

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG, E_STATE = -1, -3
B, LD, STEPS = 5, 8, 60
CFGS = [br.cfg(0.5), br.cfg(0.7, 0.3), br.cfg(0.7, 0.3, min_on=5), br.cfg(0.7, 0.3, min_off=4), br.cfg(0.7, 0.3, pad_on=3),
        br.cfg(0.7, 0.3, pad_off=3), br.cfg(0.7, 0.3, 3, 4, 2, 5), br.cfg(0.6, 0.25, min_on=12), br.cfg(0.3, 0.3, 0, 1, 2, 2)]
IDS = ["-".join(str(v) for v in q) for q in CFGS]
KEYS = ("events", "ev_counts", "active", "labels", "lab_counts")


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def _levels(q):
    """(HI values, MID values, LO values): the thresholds themselves, the f32 just below each, and NaN among them."""
    on, off = np.float32(q.onset), np.float32(q.offset)
    below = lambda v: np.nextafter(v, np.float32(-1))
    return [0.95, on, np.nan], ([below(on), off] if off < on else []), [0.02, below(off)]


def _stream_of(rng, n, q):
    """n block-structured probabilities: HI / MID / LO blocks with lengths drawn around D, min_on and min_off, so that fills, drops and
    confirmations are decided both ways."""
    hi, mid, lo = _levels(q)
    out = []
    while len(out) < n:
        around = (hr.gap(q), q.min_on, q.min_off, 1, 3, hr.gap(q) + 1)[int(rng.integers(0, 6))]
        k = int(max(1, around + rng.integers(-1, 2)))
        kind = int(rng.integers(0, 3 if mid else 2))
        out += rng.choice([hi, lo, mid][kind], size=k).tolist()
    return np.array(out[:n], np.float32)


def _cells(counts, b, s0, s1):
    """(step, column) of every frame slot b consumes in steps s0 .. s1, in order."""
    return [(s, k) for s in range(s0, s1 + 1) for k in range(int(counts[s, b]))]


def _schedule(q, seed=11):
    """flags, counts (STEPS, B) and probs (STEPS, B, LD); NaN in every column >= n_b and every row with n_b = 0.
    slot 0  a session from step 1 to 40; one from 42 whose last run is open at its END (58)
    slot 1  a START | END one-step session (3); a session of 0 frames (6 .. 7); one from 14 dropped in mid-speech by the START of step 30;
            that one ends at 50 while an interval is pending (D >= 1)
    slot 2  random churn
    slot 3  the session every slot holds after reset, fed without a START, ended at 45 with a one-frame candidate as its last frame
            (unconfirmed when min_on > pad_on + 1); then nothing
    slot 4  idle throughout"""
    rng = np.random.default_rng(seed + 1000 * CFGS.index(q) if q in CFGS else seed)
    hi, mid, lo = _levels(q)
    D = hr.gap(q)
    flags = np.zeros((STEPS, B), np.uint8)
    counts = rng.integers(0, LD + 1, (STEPS, B)).astype(np.int32)
    flags[1, 0], flags[40, 0], flags[42, 0], flags[58, 0] = 1, 2, 1, 2
    counts[0, 0] = counts[41, 0] = counts[59, 0] = 0                 # slot 0 holds the empty session there: feed it nothing
    flags[3, 1] = 3
    flags[6, 1], flags[7, 1] = 1, 2
    counts[0:3, 1] = counts[4:14, 1] = 0
    flags[14, 1], flags[30, 1], flags[50, 1] = 1, 1, 2
    counts[51:, 1] = 0
    counts[27:30, 1] = counts[48:51, 1] = LD
    live = False
    for s in range(STEPS):
        r = rng.random()
        if not live and r < 0.2:
            flags[s, 2] = 3 if rng.random() < 0.2 else 1
            live = flags[s, 2] == 1
        elif live and r < 0.05:
            flags[s, 2] = 1
        elif live and r < 0.15:
            flags[s, 2], live = 2, False
        if not live and not flags[s, 2]:
            counts[s, 2] = 0
    flags[45, 3] = 2
    counts[46:, 3] = 0
    counts[43:46, 3] = LD
    counts[:, 4] = 0
    probs = np.full((STEPS, B, LD), np.nan, np.float32)
    for b in range(B):
        cells = _cells(counts, b, 0, STEPS - 1)
        for (s, k), v in zip(cells, _stream_of(rng, len(cells), q)):
            probs[s, b, k] = v

    def tail(b, s0, s1, values):
        cells = _cells(counts, b, s0, s1)[-len(values):]
        for (s, k), v in zip(cells, values[-len(cells):]):
            probs[s, b, k] = v
    long_run = [0.95] * (q.min_on + LD + 3)                          # confirmed a step before it ends
    tail(0, 42, 58, long_run)                                        # in speech at END
    tail(1, 14, 29, long_run)                                        # in speech when the START of step 30 drops it
    tail(1, 30, 50, long_run + [0.02] * max(1, min(D, 4)))           # a run closed <= D frames before END: pending (D >= 1)
    tail(3, 0, 45, [0.02] * min(D + 2, 20) + [0.95])                 # a candidate of one frame as the session's last
    if mid:                                                          # MID runs across the boundary of steps 20 | 21, in either state
        for b, first in ((0, 0.95), (3, 0.02)):
            counts[20:22, b] = LD
            probs[20, b], probs[21, b] = [first] * 4 + [mid[0]] * 4, [mid[1]] * 3 + [0.95, 0.02] * 2 + [mid[0]]
    return flags, counts, probs


def _open(rt, nb, ld, q, max_events=None):
    return rt.endpoint_hyst_open(nb, ld, q.onset, q.offset, q.min_on, q.min_off, q.pad_on, q.pad_off, max_events=max_events)


def _run(rt, probs, counts, flags, q, max_events=None, graph_at=None, null_flags=False, ep=None, enqueue=None, step=None):
    """Every step of an endpointer -> dict of host arrays indexed [step]: events, ev_counts, active, labels, lab_counts; and its state.
    ep / enqueue / step: another endpointer's (the median one's), default the hysteresis endpointer under q."""
    steps, nb, ld = probs.shape
    ep = _open(rt, nb, ld, q, max_events) if ep is None else ep
    enqueue, step = enqueue or rt._endpoint_hyst_enqueue, step or rt.endpoint_hyst_step
    dp, dc = torch.from_numpy(probs).to(DEV), torch.from_numpy(counts).to(DEV)
    got = {k: [] for k in KEYS}
    graph = None
    pb, cb, fb = torch.empty_like(dp[0]), torch.empty_like(dc[0]), torch.zeros(nb, dtype=torch.uint8, device=DEV)
    for s in range(steps):
        fl = flags[s]
        if graph_at is not None and s >= graph_at:
            pb.copy_(dp[s]); cb.copy_(dc[s]); fb.copy_(torch.from_numpy(fl).to(DEV))
            if graph is None:
                cur = torch.cuda.current_stream(DEV)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    r = enqueue(ep, pb.data_ptr(), cb.data_ptr(), fb.data_ptr())
                assert r == 0
                torch.cuda.current_stream(DEV).wait_stream(cur)
            graph.replay()
        elif null_flags and not fl.any():
            step(ep, dp[s], dc[s])
        else:
            step(ep, dp[s], dc[s], start=fl & 1 == 1, end=fl & 2 == 2)
        for k in KEYS:
            got[k].append(ep[k].clone())
    torch.cuda.synchronize()
    return {k: torch.stack(v).cpu().numpy() for k, v in got.items()}, ep


def _check_steps(got, want, max_events):
    for s, row in enumerate(want):
        for b, (y, ev, active) in enumerate(row):
            assert got["ev_counts"][s, b] == len(ev), (s, b, ev)
            keep = min(len(ev), max_events)
            assert got["events"][s, b, :keep].tolist() == [list(e) for e in ev[:keep]], (s, b, ev)
            assert got["active"][s, b] == active, (s, b)
            assert got["lab_counts"][s, b] == len(y), (s, b)
            assert np.array_equal(got["labels"][s, b, :len(y)], y), (s, b)


def _session_outputs(got, b, s0, s1):
    labs = [got["labels"][s, b, :got["lab_counts"][s, b]] for s in range(s0, s1 + 1)]
    evs = [tuple(e) for s in range(s0, s1 + 1) for e in got["events"][s, b, :got["ev_counts"][s, b]].tolist()]
    return np.concatenate(labs), evs


_CACHE = {}


def _case(rt, q):
    """The schedule of q, its simulation (computed once, shared, never written) and the eager run on the device."""
    if q not in _CACHE:
        flags, counts, probs = _schedule(q)
        got, _ = _run(rt, probs, counts, flags, q, null_flags=True)
        _CACHE[q] = (flags, counts, probs, hr.simulate(probs, counts, flags, q), got)
    return _CACHE[q]


def _mid_crossings(flags, counts, probs, q):
    """The carried states {0, 1} with which a MID run crosses a step boundary inside a session."""
    on, off = np.float32(q.onset), np.float32(q.offset)
    seen = set()
    for b, s0, s1, _ in er.sessions(counts, flags):
        cells = _cells(counts, b, s0, s1)
        row = np.array([probs[s, b, k] for s, k in cells], np.float32)
        st = br.states(row, len(row), q)
        with np.errstate(invalid="ignore"):
            is_mid = ~(row < off) & (row < on)
        for i in range(1, len(cells)):
            if cells[i][0] != cells[i - 1][0] and is_mid[i] and is_mid[i - 1]:
                seen.add(st[i])
    return seen


def test_schedule_holds_what_it_promises():
    dropped = filled = candidate = 0
    for q in CFGS:
        flags, counts, probs = _schedule(q)
        D = hr.gap(q)
        assert counts.min() == 0 and counts.max() == LD and not flags[:, 4].any() and counts[:, 4].sum() == 0
        cols = np.arange(LD)[None, None, :]
        assert np.isnan(probs[cols >= counts[:, :, None]]).all()
        sess = er.sessions(counts, flags)
        rows = {(b, s0): er.session_row(probs, counts, b, s0, s1) for b, s0, s1, _ in sess}
        assert (1, 3, 3, True) in sess and (1, 14, 29, False) in sess and (3, 0, 45, True) in sess and (1, 6, 7, True) in sess
        assert len(rows[(1, 6)]) == 0
        want = hr.simulate(probs, counts, flags, q)
        assert want[29][1][2] == 1 and not any(e[0] == hr.END for e in want[30][1][1][:1])       # dropped in speech, no closing event
        assert want[57][0][2] == 1 and want[58][0][1][-1] == (hr.END, len(rows[(0, 42)]))        # open at END: closed at n
        if D:
            assert want[49][1][2] == 1 and want[50][1][1][-1][0] == hr.END and want[50][1][1][-1][1] <= len(rows[(1, 30)])   # pending at END
        if q.min_on > q.pad_on + 1 and D == 0:                                                   # the last candidate: unconfirmed at END, no events
            n3 = len(rows[(3, 0)])
            assert br.row(rows[(3, 0)], n3, q._replace(min_on=0))[-1] == (n3 - 1, n3) and (br.row(rows[(3, 0)], n3, q) or [(0, 0)])[-1][1] < n3
            assert not want[45][3][1] or want[45][3][1][-1][1] < n3
        for v in _levels(q)[0][1:] + _levels(q)[1] + _levels(q)[2][1:]:                           # onset, below it, offset, below it, NaN
            assert (np.isnan(probs).sum() > (probs.shape[0] * B * LD - counts.sum())) if np.isnan(v) else (probs == v).any(), v
        for row in rows.values():
            dropped += len(br.row(row, len(row), q._replace(min_on=0))) - len(br.row(row, len(row), q))
            if q.pad_on == q.pad_off == 0 and q.min_off > 1:
                filled += len(br.row(row, len(row), q._replace(min_off=0, min_on=0))) - len(br.row(row, len(row), q._replace(min_on=0)))
        candidate += sum(w[b][2] == 2 for w in want for b in range(B))
        if q.offset < q.onset:
            assert _mid_crossings(flags, counts, probs, q) == {0, 1}
        assert {w[b][2] for w in want for b in range(B)} >= {0, 1}
        if q in (CFGS[0], CFGS[3]):
            assert max(len(w[b][1]) for w in want for b in range(B)) >= 2                        # what the max_events = 1 test overflows
    assert dropped > 0 and filled > 0 and candidate > 0


@pytest.mark.parametrize("q", CFGS, ids=IDS)
def test_every_step_equals_the_simulator(rt, q):
    flags, counts, probs, want, got = _case(rt, q)
    _check_steps(got, want, LD + 1)
    assert got["ev_counts"].max() <= LD + 1 and got["lab_counts"].max() <= LD + hr.lag(q)
    assert not got["ev_counts"][:, 4].any() and not got["active"][:, 4].any() and not got["lab_counts"][:, 4].any()


@pytest.mark.parametrize("q", CFGS, ids=IDS)
def test_ended_sessions_equal_binarize_on_the_device(rt, q):
    """Interval list and label bytes of uvad_binarize over each ended session's whole row."""
    flags, counts, probs, _, got = _case(rt, q)
    sess = [v for v in er.sessions(counts, flags) if v[3]]
    rows = [er.session_row(probs, counts, b, s0, s1) for b, s0, s1, _ in sess]
    T = max(1, max(len(r) for r in rows))
    mat = np.zeros((len(rows), T), np.float32)
    for i, r in enumerate(rows):
        mat[i, :len(r)] = r
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)
    st = rt.binarize_open(**q._asdict())
    labels, _, cn = rt.binarize(torch.from_numpy(mat).to(DEV), lengths=lens, state=st)
    offline_iv, labels, cn = rt.binarize_read(st), labels.cpu().numpy(), cn.cpu().numpy()
    assert cn.sum() > 0
    for i, ((b, s0, s1, _), row) in enumerate(zip(sess, rows)):
        labs, evs = _session_outputs(got, b, s0, s1)
        assert len(offline_iv[i]) == cn[i]
        assert evs == hr.events_of(offline_iv[i]), (b, s0)
        assert labs.tobytes() == labels[i, :len(row)].tobytes(), (b, s0)


def _recut(sess_rows, cut, rng):
    """Per slot a list of (row, ended) sessions -> flags, counts, probs of a schedule that feeds them `cut` frames at a time (0: random)."""
    plans = []
    for rows in sess_rows:
        plan = []                                                    # (flag, frames)
        for row, ended in rows:
            sizes, left = [], len(row)
            while left > 0 or not sizes:
                k = min(left, cut if cut else int(rng.integers(0, LD + 1)))
                sizes.append(k)
                left -= k
            pos = 0
            for i, k in enumerate(sizes):
                plan.append(((1 if i == 0 else 0) | (2 if ended and i == len(sizes) - 1 else 0), row[pos:pos + k]))
                pos += k
        plans.append(plan)
    steps = max(len(p) for p in plans)
    flags, counts = np.zeros((steps, len(plans)), np.uint8), np.zeros((steps, len(plans)), np.int32)
    probs = np.full((steps, len(plans), LD), np.nan, np.float32)
    for b, plan in enumerate(plans):
        for s, (fl, fr) in enumerate(plan):
            flags[s, b], counts[s, b] = fl, len(fr)
            probs[s, b, :len(fr)] = fr
    return flags, counts, probs


@pytest.mark.parametrize("q", [CFGS[2], CFGS[6]], ids=[IDS[2], IDS[6]])
def test_cut_invariance(rt, q):
    """The sessions of the schedule as they were cut, fed 1 frame per step and fed a random 0 .. 8 per step: identical labels and events."""
    flags, counts, probs, _, got = _case(rt, q)
    per_slot = [[] for _ in range(B)]
    first = []
    for b, s0, s1, ended in er.sessions(counts, flags):
        if len(_cells(counts, b, s0, s1)) or ended:
            per_slot[b].append((er.session_row(probs, counts, b, s0, s1), ended))
            y, ev = _session_outputs(got, b, s0, s1)
            first.append((y.tobytes(), ev))
    rng = np.random.default_rng(CFGS.index(q))
    seen = [first]
    for cut in (1, 0):
        f2, c2, p2 = _recut(per_slot, cut, rng)
        again, _ = _run(rt, p2, c2, f2, q)
        _check_steps(again, hr.simulate(p2, c2, f2, q), LD + 1)
        outs = [_session_outputs(again, b, s0, s1) for b, s0, s1, _ in er.sessions(c2, f2) if f2[s0, b] & 1]
        seen.append([(y.tobytes(), ev) for y, ev in outs])
    want = [(hr.whole(row, q), ended) for rows in per_slot for row, ended in rows]
    assert len(want) == len(seen[0]) == len(seen[1]) == len(seen[2])
    for i, ((y, iv), ended) in enumerate(want):
        if ended:
            assert seen[0][i] == seen[1][i] == seen[2][i] == (y.tobytes(), hr.events_of(iv)), i
        else:                                                        # still running: what is final so far depends on no cut
            assert seen[0][i] == seen[1][i] == seen[2][i], i


@pytest.mark.parametrize("q", [CFGS[0], CFGS[6]], ids=[IDS[0], IDS[6]])
def test_padding_columns_and_idle_rows_are_never_read(rt, q):
    flags, counts, probs, _, got = _case(rt, q)
    pad = np.arange(LD)[None, None, :] >= counts[:, :, None]
    for poison in (0.0, np.inf):
        p2 = probs.copy()
        p2[pad] = poison
        again, _ = _run(rt, p2, counts, flags, q, null_flags=True)
        for k in got:
            assert again[k].tobytes() == got[k].tobytes(), (poison, k)


@pytest.mark.parametrize("q", [CFGS[0], CFGS[3]], ids=[IDS[0], IDS[3]])
def test_max_events_1_counts_truly_and_harms_nothing(rt, q):
    flags, counts, probs, want, full = _case(rt, q)
    got, _ = _run(rt, probs, counts, flags, q, max_events=1, null_flags=True)
    assert got["events"].shape[2] == 1 and full["ev_counts"].max() > 1
    assert np.array_equal(got["ev_counts"], full["ev_counts"])
    _check_steps(got, want, 1)
    for k in ("active", "labels", "lab_counts"):
        assert got[k].tobytes() == full[k].tobytes(), k


@pytest.mark.parametrize("q", [CFGS[1], CFGS[6]], ids=[IDS[1], IDS[6]])
def test_one_graph_captured_at_step_3_replays_every_later_step(rt, q):
    flags, counts, probs, _, eager = _case(rt, q)
    got, _ = _run(rt, probs, counts, flags, q, graph_at=3)
    for k in eager:
        assert got[k].tobytes() == eager[k].tobytes(), k


@pytest.mark.parametrize("P,min_off,thr", [(0, 0, 0.5), (2, 1, 0.3), (7, 0, 0.5)])
def test_every_step_equals_the_median_endpointer_at_kernel_1(rt, P, min_off, thr):
    q = br.cfg(thr, thr, 0, min_off, P, P)
    flags, counts, probs = _schedule(q)
    got, _ = _run(rt, probs, counts, flags, q, null_flags=True)
    med, _ = _run(rt, probs, counts, flags, q, null_flags=True, ep=rt.endpoint_open(B, LD, kernel=1, pad=P, threshold=thr),
                  enqueue=rt._endpoint_enqueue, step=rt.endpoint_step)
    assert got["ev_counts"].sum() > 4
    assert np.array_equal(got["ev_counts"], med["ev_counts"]) and np.array_equal(got["active"], med["active"])
    for s in range(STEPS):
        for b in range(B):
            n = got["ev_counts"][s, b]
            assert got["events"][s, b, :n].tolist() == med["events"][s, b, :n].tolist(), (s, b)


def test_three_ballot_words_the_last_partial(rt):
    """B = 2, ld_in = 130, 6 steps: a MID run that crosses both word boundaries (frames 63 | 64 and 127 | 128) and the step boundary, in
    state 1 in slot 0 and in state 0 in slot 1; counts of 130, 129, 128, 65, 64 and 1 frames."""
    q = br.cfg(0.7, 0.3, 3, 4, 2, 5)
    ld, nb = 130, 2
    rng = np.random.default_rng(130)
    counts = np.array([[130, 130], [130, 129], [128, 65], [64, 1], [130, 130], [130, 0]], np.int32)
    flags = np.zeros((6, nb), np.uint8)
    flags[0, :], flags[5, :] = 1, 2
    probs = np.full((6, nb, ld), np.nan, np.float32)
    for b in range(nb):
        cells = _cells(counts, b, 0, 5)
        for (s, k), v in zip(cells, _stream_of(rng, len(cells), q)):
            probs[s, b, k] = v
    for b, first in ((0, 0.95), (1, 0.02)):
        probs[0, b, 40:50] = first
        probs[0, b, 50:130] = 0.5                                    # MID across 63 | 64, 127 | 128 and into the next step
        probs[1, b, 0:70] = 0.5                                      # ... and across the next step's 63 | 64
        probs[1, b, 70:80] = 0.98 - first
    assert _mid_crossings(flags, counts, probs, q) == {0, 1}
    got, _ = _run(rt, probs, counts, flags, q)
    want = hr.simulate(probs, counts, flags, q)
    _check_steps(got, want, ld + 1)
    for b in range(nb):
        row = er.session_row(probs, counts, b, 0, 5)
        labs, evs = _session_outputs(got, b, 0, 5)
        y, iv = hr.whole(row, q)
        assert labs.tobytes() == y.tobytes() and evs == hr.events_of(iv) and len(iv) > 3


def test_min_on_300_pad_on_40_ld_in_3(rt):
    """A long lag against tiny steps: candidates live for a hundred steps before they are confirmed or dropped."""
    q, ld = br.cfg(0.7, 0.3, 300, 0, 40, 0), 3
    rng = np.random.default_rng(300)
    # runs of 259 (+ 40 = 299: dropped), 260 (kept), 30 and 200 frames 40 apart (merged by the pad: 270 + 40 kept), 100 (dropped), 280 open at END
    row = np.repeat([0.1, 0.9, 0.1, 0.9, 0.1, 0.9, 0.1, 0.9, 0.1, 0.9, 0.1, 0.9], [50, 259, 100, 260, 90, 30, 40, 200, 60, 100, 70, 280]).astype(np.float32)
    n = len(row)
    row[rng.choice(np.flatnonzero((row > 0.5) & (np.roll(row, 1) > 0.5)), 40, replace=False)] = 0.5     # MID inside speech: holds
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(n - sum(sizes), int(rng.choice([0, 1, 2, 3], p=[0.05, 0.1, 0.15, 0.7]))))
    steps = len(sizes)
    flags, counts = np.zeros((steps, 2), np.uint8), np.zeros((steps, 2), np.int32)
    probs = np.full((steps, 2, ld), np.nan, np.float32)
    flags[0, 0], flags[-1, 0] = 1, 2
    pos = 0
    for s, k in enumerate(sizes):
        counts[s, 0] = k
        probs[s, 0, :k] = row[pos:pos + k]
        pos += k
    got, ep = _run(rt, probs, counts, flags, q)
    assert ep["lag"] == 340 and ep["labels"].shape[1] == ld + 340
    labs, evs = _session_outputs(got, 0, 0, steps - 1)
    want_y, want_iv = hr.whole(row, q)
    assert [hi - lo for lo, hi in want_iv] == [300, 310, 320] and len(br.row(row, n, q._replace(min_on=0))) == 5
    assert labs.tobytes() == want_y.tobytes() and evs == hr.events_of(want_iv)
    assert 300 <= got["lab_counts"].max() <= ld + 340 and not got["ev_counts"][:, 1].any()
    assert (got["active"][:, 0] == 2).sum() > 100
    _check_steps(got, hr.simulate(probs, counts, flags, q), ld + 1)


def test_refusals_leave_state_and_outputs_untouched():
    from uvad_amd import _lib
    from uvad_amd.runtime import VadRuntime
    rt = VadRuntime(DEV)          # a context of its own: none of its states has been reset except the one below
    q = CFGS[6]
    lag = hr.lag(q)
    flags, counts, probs = _schedule(q)
    got, ep = _run(rt, probs[:20], counts[:20], flags[:20], q)
    lib, ctx = rt.lib, rt.ctx
    bufs = [ep[k] for k in ("state",) + KEYS]
    before = [t.clone() for t in bufs]
    dp, dc = torch.from_numpy(probs[20]).to(DEV), torch.from_numpy(counts[20]).to(DEV)
    fl = torch.zeros(B, dtype=torch.uint8, device=DEV)
    good = dict(probs=dp.data_ptr(), ld_in=LD, counts=dc.data_ptr(), flags=fl.data_ptr(), B=B, state=ep["state"].data_ptr(),
                nbytes=ep["state"].numel(), events=ep["events"].data_ptr(), max_events=ep["max_events"], ev_counts=ep["ev_counts"].data_ptr(),
                active=ep["active"].data_ptr(), labels=ep["labels"].data_ptr(), ld_lab=LD + lag, lab_counts=ep["lab_counts"].data_ptr())

    def step(**kw):
        a = dict(good, **kw)
        return lib.uvad_endpoint_hyst_step(ctx, a["probs"], a["ld_in"], a["counts"], a["flags"], a["B"], a["state"], a["nbytes"], a["events"],
                                           a["max_events"], a["ev_counts"], a["active"], a["labels"], a["ld_lab"], a["lab_counts"], None)
    other = torch.zeros(ep["state"].numel(), dtype=torch.uint8, device=DEV)           # big enough, never reset
    median = rt.endpoint_open(B, LD, kernel=1)                                        # reset, but by the other endpointer
    cases = [(dict(probs=None), E_ARG), (dict(counts=None), E_ARG), (dict(ev_counts=None), E_ARG), (dict(B=0), E_ARG), (dict(ld_in=0), E_ARG),
             (dict(ld_in=(1 << 18) + 1), E_ARG), (dict(events=None), E_ARG), (dict(max_events=-1), E_ARG), (dict(ld_lab=LD + lag - 1), E_ARG),
             (dict(lab_counts=None), E_ARG), (dict(nbytes=ep["state"].numel() - 1), E_ARG), (dict(state=None), E_ARG),
             (dict(state=other.data_ptr()), E_STATE), (dict(state=median["state"].data_ptr()), E_STATE), (dict(B=B - 1), E_STATE),
             (dict(B=B + 1), E_STATE)]
    for kw, code in cases:
        assert step(**kw) == code, kw
    nbytes = ep["state"].numel()
    M = 1 << 20
    for cfg in ((float("nan"), 0.3, 0, 0, 0, 0), (0.7, float("inf"), 0, 0, 0, 0), (0.3, 0.7, 0, 0, 0, 0), (0.7, 0.3, -1, 0, 0, 0),
                (0.7, 0.3, 0, M + 1, 0, 0), (0.7, 0.3, 0, 0, -1, 0), (0.7, 0.3, 0, 0, 0, M + 1)):
        assert lib.uvad_endpoint_hyst_reset(ctx, ep["state"].data_ptr(), nbytes, B, C.byref(_lib.BinarizeCfg(*cfg)), None) == E_ARG, cfg
    cfg = _lib.BinarizeCfg(*q)
    assert lib.uvad_endpoint_hyst_reset(ctx, ep["state"].data_ptr(), nbytes - 1, B, C.byref(cfg), None) == E_ARG
    assert lib.uvad_endpoint_hyst_reset(ctx, ep["state"].data_ptr(), nbytes, 0, C.byref(cfg), None) == E_ARG
    assert lib.uvad_endpoint_hyst_reset(ctx, ep["state"].data_ptr(), nbytes, B, None, None) == E_ARG
    for bad in ({"onset": 0.3, "offset": 0.7}, {"pad_on": -1}, {"onset": float("inf")}, {"min_on": M + 1}):
        with pytest.raises(ValueError):
            rt.endpoint_hyst_open(B, LD, **bad)
    torch.cuda.synchronize()
    for t, t0 in zip(bufs, before):
        assert torch.equal(t, t0)
    assert not other.any()
    # ... and the stream goes on as if nothing had happened
    want = hr.simulate(probs[:21], counts[:21], flags[:21], q)
    assert step() == 0
    torch.cuda.synchronize()
    for b in range(B):
        y, ev, active = want[20][b]
        assert ep["ev_counts"][b].item() == len(ev) and ep["active"][b].item() == active and ep["lab_counts"][b].item() == len(y)
        assert ep["labels"][b, :len(y)].cpu().numpy().tolist() == y.tolist()
    # optional outputs may all be NULL
    assert step(events=None, max_events=0, active=None, labels=None, ld_lab=0, lab_counts=None, flags=None) == 0
    torch.cuda.synchronize()
    rt.close()
