"""GPU tests (-m gpu) of the live endpointer (uvad_endpoint_*, VadRuntime.endpoint_*): B = 5 slots, ld_in = 8, 60 steps of 0 .. 8 frames per
slot, median kernels {1, 3, 25} x pads {0, 1, 7}, thresholds 0.5 and 0.3.

  offline     per session, the labels finalised step by step equal uvad_median_filter_lens over the assembled row byte for byte (0.5) and
              the numpy reference (0.3); at pad 0 the events are the runs of uvad_label_runs_lens on those labels
  step-wise   every step's events, counts, active byte and labels equal the simulator of tests/endpoint_ref.py, at every pad
  cuts        the same sessions fed 1 frame, 8 frames or a random number of frames at a time give the same labels and events
  isolation   NaN, 0.0 or +Inf in columns >= n_b and in rows with n_b = 0 change no output byte
  overflow    max_events = 1 counts truly, keeps the first event and harms no state
  one graph   a graph captured around step 3 replays every later step to the eager run's bytes
  plus every refusal (state and outputs untouched) and K = 255, pad 300, ld_in = 3: history longer than a step, pad longer than history.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import endpoint_ref as er

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG, E_STATE = -1, -3
B, LD, STEPS = 5, 8, 60
KERNELS, PADS = [1, 3, 25], [0, 1, 7]
GRID = [(K, P) for K in KERNELS for P in PADS]


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def _stream_of(rng, n, K, P, thr):
    """n block-structured probabilities: speech / silence blocks with lengths drawn around h and around 2 P, so that medians flip and merges
    are decided both ways; values exactly thr (speech) and a few NaN (speech) inside."""
    h, out, v = K // 2, [], int(rng.integers(0, 2))
    lo = np.nextafter(np.float32(thr), np.float32(0))
    while len(out) < n:
        around = (h, 2 * P, h + 1, 2 * P + 1, 1, 3)[int(rng.integers(0, 6))]
        k = int(max(1, around + rng.integers(-1, 2)))
        vals = rng.choice([0.9, thr, np.nan] if v else [0.1, lo], size=k, p=[0.7, 0.2, 0.1] if v else [0.7, 0.3])
        out += vals.tolist()
        v ^= 1
    return np.array(out[:n], np.float32)


def _cells(counts, b, s0, s1):
    """(step, column) of every frame slot b consumes in steps s0 .. s1, in order."""
    return [(s, k) for s in range(s0, s1 + 1) for k in range(int(counts[s, b]))]


def _schedule(K, P, thr, seed=7):
    """flags, counts (STEPS, B) and probs (STEPS, B, LD); NaN in every column >= n_b and every row with n_b = 0.
    slot 0  a session from step 1 to 40; one from 42 whose last run is open at its END (58)
    slot 1  a START | END one-step session (3); a session of 0 frames (6 .. 7); one shorter than h + 1 (10 .. 11); one from 14 dropped in
            mid-speech by the START of step 30; that one ends at 50 while an interval is pending
    slot 2  random churn
    slot 3  the session every slot holds after reset, fed without a START, ended at 45; then nothing
    slot 4  idle throughout"""
    rng = np.random.default_rng(seed + 100 * K + P)
    h = K // 2
    flags = np.zeros((STEPS, B), np.uint8)
    counts = rng.integers(0, LD + 1, (STEPS, B)).astype(np.int32)
    flags[1, 0], flags[40, 0], flags[42, 0], flags[58, 0] = 1, 2, 1, 2
    counts[0, 0] = counts[41, 0] = counts[59, 0] = 0                 # slot 0 holds the empty session there: feed it nothing
    flags[3, 1] = 3
    flags[6, 1], flags[7, 1] = 1, 2
    counts[4:10, 1] = 0
    counts[0:3, 1] = 0
    flags[10, 1], flags[11, 1] = 1, 2
    counts[10, 1], counts[11, 1] = min(h, LD), 0                     # h frames at most: no label is final before the END
    counts[12:14, 1] = 0
    flags[14, 1], flags[30, 1], flags[50, 1] = 1, 1, 2
    counts[51:, 1] = 0
    counts[27:30, 1] = LD
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
    counts[:, 4] = 0
    probs = np.full((STEPS, B, LD), np.nan, np.float32)
    for b in range(B):
        cells = _cells(counts, b, 0, STEPS - 1)
        vals = _stream_of(rng, len(cells), K, P, thr)
        for (s, k), v in zip(cells, vals):
            probs[s, b, k] = v

    def tail(b, s0, s1, values):
        cells = _cells(counts, b, s0, s1)[-len(values):]
        for (s, k), v in zip(cells, values[-len(cells):]):
            probs[s, b, k] = v
    tail(0, 42, 58, [0.9] * (K + 2))                                 # in speech at END
    tail(1, 14, 29, [0.9] * (K + 2))                                 # in speech when the START of step 30 drops it
    tail(1, 30, 50, [0.9] * (K + 2) + [0.1] * max(1, P))             # a run closed max(1, P) <= 2 P frames before END: pending (P >= 1)
    return flags, counts, probs


def _run(rt, probs, counts, flags, K, P, thr, max_events=None, graph_at=None, null_flags=False):
    """Every step of an endpointer -> dict of host arrays indexed [step]: events, ev_counts, active, labels, lab_counts; and its state."""
    steps, nb, ld = probs.shape
    ep = rt.endpoint_open(nb, ld, kernel=K, pad=P, threshold=thr, max_events=max_events)
    dp, dc = torch.from_numpy(probs).to(DEV), torch.from_numpy(counts).to(DEV)
    keys = ("events", "ev_counts", "active", "labels", "lab_counts")
    got = {k: [] for k in keys}
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
                    r = rt._endpoint_enqueue(ep, pb.data_ptr(), cb.data_ptr(), fb.data_ptr())
                assert r == 0
                torch.cuda.current_stream(DEV).wait_stream(cur)
            graph.replay()
        elif null_flags and not fl.any():
            rt.endpoint_step(ep, dp[s], dc[s])
        else:
            rt.endpoint_step(ep, dp[s], dc[s], start=fl & 1 == 1, end=fl & 2 == 2)
        for k in keys:
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


def _case(rt, K, P, thr):
    key = (K, P, thr)
    if key not in _CACHE:
        flags, counts, probs = _schedule(K, P, thr)
        got, _ = _run(rt, probs, counts, flags, K, P, thr, null_flags=True)
        _CACHE[key] = (flags, counts, probs, got)
    return _CACHE[key]


def test_schedule_holds_what_it_promises():
    for K, P in GRID:
        flags, counts, probs = _schedule(K, P, 0.5)
        h = K // 2
        assert counts.min() == 0 and counts.max() == LD and not flags[:, 4].any() and counts[:, 4].sum() == 0
        cols = np.arange(LD)[None, None, :]
        assert np.isnan(probs[cols >= counts[:, :, None]]).all()
        sess = er.sessions(counts, flags)
        rows = {(b, s0): er.session_row(probs, counts, b, s0, s1) for b, s0, s1, _ in sess}
        assert (1, 3, 3, True) in sess and (1, 14, 29, False) in sess and (3, 0, 45, True) in sess
        assert len(rows[(1, 6)]) == 0 and len(rows[(1, 10)]) <= h
        want = er.simulate(probs, counts, flags, K, P)
        assert want[29][1][2] == 1 and not any(e[0] == er.END for e in want[30][1][1][:1])       # dropped in speech, no closing event
        assert want[57][0][2] == 1 and want[58][0][1][-1] == (er.END, len(rows[(0, 42)]))        # open at END: closed at n
        if P:
            assert want[49][1][2] == 1 and want[50][1][1][-1][1] <= len(rows[(1, 30)])           # pending at END
        assert max(len(w[b][1]) for w in want for b in range(B)) >= (2 if K == 1 else 1)


@pytest.mark.parametrize("K,P", GRID)
@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_every_step_equals_the_simulator(rt, K, P, thr):
    flags, counts, probs, got = _case(rt, K, P, thr)
    _check_steps(got, er.simulate(probs, counts, flags, K, P, thr), LD + K // 2 + 2)
    assert not got["ev_counts"][:, 4].any() and not got["active"][:, 4].any() and not got["lab_counts"][:, 4].any()


@pytest.mark.parametrize("K,P", GRID)
@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_sessions_equal_the_offline_kernels(rt, K, P, thr):
    """Concatenated labels == uvad_median_filter_lens of the whole row (0.5; a session that was dropped or is still running has its
    labels up to n - h) / the numpy reference (0.3); at pad 0 the events are uvad_label_runs_lens on the labels; at every pad the events
    of an ended session are START / END of the reference's merged intervals."""
    flags, counts, probs, got = _case(rt, K, P, thr)
    h = K // 2
    sess = er.sessions(counts, flags)
    rows = [er.session_row(probs, counts, b, s0, s1) for b, s0, s1, _ in sess]
    T = max(1, max(len(r) for r in rows))
    mat = np.zeros((len(rows), T), np.float32)
    for i, r in enumerate(rows):
        mat[i, :len(r)] = r
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)
    offline = rt.median_filter(torch.from_numpy(mat).to(DEV), K, lengths=lens)
    runs, nruns = rt.label_runs(offline, lengths=lens)
    offline, runs, nruns = offline.cpu().numpy(), runs.cpu().numpy(), nruns.cpu().numpy()
    for i, ((b, s0, s1, ended), row) in enumerate(zip(sess, rows)):
        labs, evs = _session_outputs(got, b, s0, s1)
        n = len(row)
        final = n if ended else max(0, n - h)
        want_y, want_iv = er.whole(row, K, P, thr)
        assert len(labs) == final, (b, s0)
        assert np.array_equal(labs, want_y[:final]), (b, s0)
        if thr == 0.5:
            assert labs.tobytes() == offline[i, :final].tobytes(), (b, s0)
        if ended:
            assert evs == er.events_of(want_iv), (b, s0)
            if P == 0 and thr == 0.5:
                assert evs == [(k, int(f)) for pair in runs[i, :nruns[i]] for k, f in zip((er.START, er.END), pair)], (b, s0)


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


@pytest.mark.parametrize("K,P", GRID)
def test_cut_invariance(rt, K, P):
    """The sessions of the schedule, fed 1 frame per step, 8 per step and a random 0 .. 8 per step: identical labels and events."""
    flags, counts, probs = _schedule(K, P, 0.5)
    per_slot = [[] for _ in range(B)]
    for b, s0, s1, ended in er.sessions(counts, flags):
        per_slot[b].append((er.session_row(probs, counts, b, s0, s1), ended))
    rng = np.random.default_rng(K + P)
    seen = []
    for cut in (1, LD, 0):
        f2, c2, p2 = _recut(per_slot, cut, rng)
        got, _ = _run(rt, p2, c2, f2, K, P, 0.5)
        _check_steps(got, er.simulate(p2, c2, f2, K, P), LD + K // 2 + 2)
        outs = [_session_outputs(got, b, s0, s1) for b, s0, s1, _ in er.sessions(c2, f2) if f2[s0, b] & 1]
        seen.append([(y.tobytes(), ev) for y, ev in outs])
    assert seen[0] == seen[1] == seen[2]
    want = [er.whole(row, K, P) for rows in per_slot for row, _ in rows]
    ended = [e for rows in per_slot for _, e in rows]
    assert len(want) == len(seen[0])
    for (y, iv), (yb, ev), e in zip(want, seen[0], ended):
        if e:
            assert yb == y.tobytes() and ev == er.events_of(iv)


@pytest.mark.parametrize("K,P", [(1, 0), (3, 1), (25, 7)])
def test_padding_columns_and_idle_rows_are_never_read(rt, K, P):
    flags, counts, probs, got = _case(rt, K, P, 0.5)
    pad = np.arange(LD)[None, None, :] >= counts[:, :, None]
    for poison in (0.0, np.inf):
        p2 = probs.copy()
        p2[pad] = poison
        again, _ = _run(rt, p2, counts, flags, K, P, 0.5, null_flags=True)
        for k in got:
            assert again[k].tobytes() == got[k].tobytes(), (poison, k)


@pytest.mark.parametrize("K,P", [(1, 0), (3, 1)])
def test_max_events_1_counts_truly_and_harms_nothing(rt, K, P):
    flags, counts, probs, full = _case(rt, K, P, 0.5)
    got, _ = _run(rt, probs, counts, flags, K, P, 0.5, max_events=1, null_flags=True)
    assert got["events"].shape[2] == 1 and full["ev_counts"].max() > 1
    assert np.array_equal(got["ev_counts"], full["ev_counts"])
    _check_steps(got, er.simulate(probs, counts, flags, K, P), 1)
    for k in ("active", "labels", "lab_counts"):
        assert got[k].tobytes() == full[k].tobytes(), k


@pytest.mark.parametrize("K,P", [(3, 0), (25, 7)])
def test_one_graph_captured_at_step_3_replays_every_later_step(rt, K, P):
    flags, counts, probs, eager = _case(rt, K, P, 0.5)
    got, _ = _run(rt, probs, counts, flags, K, P, 0.5, graph_at=3)
    for k in eager:
        assert got[k].tobytes() == eager[k].tobytes(), k


def test_refusals_leave_state_and_outputs_untouched():
    from uvad_amd import _lib
    from uvad_amd.runtime import VadRuntime
    rt = VadRuntime(DEV)          # a context of its own: none of its states has been reset except the one below
    K, P = 25, 7
    flags, counts, probs = _schedule(K, P, 0.5)
    got, ep = _run(rt, probs[:20], counts[:20], flags[:20], K, P, 0.5)
    lib, ctx, h = rt.lib, rt.ctx, K // 2
    bufs = [ep[k] for k in ("state", "events", "ev_counts", "active", "labels", "lab_counts")]
    before = [t.clone() for t in bufs]
    dp, dc = torch.from_numpy(probs[20]).to(DEV), torch.from_numpy(counts[20]).to(DEV)
    fl = torch.zeros(B, dtype=torch.uint8, device=DEV)
    good = dict(probs=dp.data_ptr(), ld_in=LD, counts=dc.data_ptr(), flags=fl.data_ptr(), B=B, state=ep["state"].data_ptr(),
                nbytes=ep["state"].numel(), events=ep["events"].data_ptr(), max_events=ep["max_events"], ev_counts=ep["ev_counts"].data_ptr(),
                active=ep["active"].data_ptr(), labels=ep["labels"].data_ptr(), ld_lab=LD + h, lab_counts=ep["lab_counts"].data_ptr())

    def step(**kw):
        a = dict(good, **kw)
        return lib.uvad_endpoint_step(ctx, a["probs"], a["ld_in"], a["counts"], a["flags"], a["B"], a["state"], a["nbytes"], a["events"],
                                      a["max_events"], a["ev_counts"], a["active"], a["labels"], a["ld_lab"], a["lab_counts"], None)
    other = torch.zeros(ep["state"].numel(), dtype=torch.uint8, device=DEV)           # big enough, never reset
    cases = [(dict(probs=None), E_ARG), (dict(counts=None), E_ARG), (dict(ev_counts=None), E_ARG), (dict(B=0), E_ARG), (dict(ld_in=0), E_ARG),
             (dict(events=None), E_ARG), (dict(ld_lab=LD + h - 1), E_ARG), (dict(lab_counts=None), E_ARG), (dict(nbytes=ep["state"].numel() - 1), E_ARG),
             (dict(state=other.data_ptr()), E_STATE), (dict(B=B - 1), E_STATE), (dict(B=B + 1), E_STATE)]
    for kw, code in cases:
        assert step(**kw) == code, kw
    nbytes = ep["state"].numel()
    for cfg in ((24, 0, 0.5), (0, 0, 0.5), (257, 0, 0.5), (25, -1, 0.5), (25, (1 << 20) + 1, 0.5), (25, 0, float("nan")), (25, 0, float("inf"))):
        assert lib.uvad_endpoint_reset(ctx, ep["state"].data_ptr(), nbytes, B, C.byref(_lib.EndpointCfg(*cfg)), None) == E_ARG, cfg
    cfg = _lib.EndpointCfg(K, P, 0.5)
    assert lib.uvad_endpoint_reset(ctx, ep["state"].data_ptr(), nbytes - 1, B, C.byref(cfg), None) == E_ARG
    assert lib.uvad_endpoint_reset(ctx, ep["state"].data_ptr(), nbytes, 0, C.byref(cfg), None) == E_ARG
    for bad in ({"kernel": 4}, {"pad": -1}, {"threshold": float("inf")}):
        with pytest.raises(ValueError):
            rt.endpoint_open(B, LD, **bad)
    torch.cuda.synchronize()
    for t, t0 in zip(bufs, before):
        assert torch.equal(t, t0)
    assert not other.any()
    # ... and the stream goes on as if nothing had happened
    want = er.simulate(probs[:21], counts[:21], flags[:21], K, P)
    assert step() == 0
    torch.cuda.synchronize()
    y, ev, active = want[20][0]
    assert ep["ev_counts"][0].item() == len(ev) and ep["active"][0].item() == active and ep["lab_counts"][0].item() == len(y)
    # optional outputs may all be NULL
    assert step(events=None, max_events=0, active=None, labels=None, ld_lab=0, lab_counts=None, flags=None) == 0
    torch.cuda.synchronize()


def test_kernel_255_pad_300_ld_in_3(rt):
    """History (254 frames) far longer than a step (3 frames) and a pad longer than the history: blocks at h = 127 and 2 P = 600."""
    K, P, ld = 255, 300, 3
    rng = np.random.default_rng(255)
    # two runs 600 frames apart (merged: 600 <= 2 P), the next 601 after (not merged); a 126-frame gap the median fills, a 127-frame burst it removes
    row = np.repeat([0.9, 0.1, 0.9, 0.1, 0.9, 0.1, 0.9, 0.1, 0.9, 0.1], [200, 600, 200, 601, 130, 126, 130, 700, 127, 100]).astype(np.float32)
    n = len(row)
    row[rng.integers(0, n, 20)] = np.nan
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
    got, _ = _run(rt, probs, counts, flags, K, P, 0.5)
    labs, evs = _session_outputs(got, 0, 0, steps - 1)
    want_y, want_iv = er.whole(row, K, P)
    assert len(want_iv) == 2 and len(er.runs(want_y)) == 3                           # merges decided both ways
    offline = rt.median_filter(torch.from_numpy(row[None]).to(DEV), K, lengths=torch.tensor([n], dtype=torch.int32, device=DEV))
    assert labs.tobytes() == offline.cpu().numpy()[0].tobytes() == want_y.tobytes()
    assert evs == er.events_of(want_iv)
    assert got["lab_counts"].max() <= ld + K // 2 and not got["ev_counts"][:, 1].any()
    _check_steps(got, er.simulate(probs, counts, flags, K, P), ld + K // 2 + 2)
