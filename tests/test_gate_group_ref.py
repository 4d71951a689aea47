"""The group gate's step rule (tests/gate_group_ref.py, restated from include/uvad.h) against its offline definition, without a GPU: however a
session's samples, best bytes and labels are cut into steps, its fragments concatenated per cut are the cuts of cuts_ref's table on the
fused labels, each gathered from the member fuse_ref's pick names on the cut's first D frames.  Also: with D >= max_len > 0 that is the
table -> pick -> gather chain as it is; with D = 1 the records are the mono gate's; under the preconditions and with the derived
histories nothing is LOST, every frame of a choice window votes and no record is truncated; how deep the reads go against the bounds; and
the hand-made cases."""
import numpy as np
import pytest

import cuts_ref
import fuse_ref
import gate_group_ref as gg
import gate_ref as gr

HOP, LEAD, TAIL = 4, 3, 3
LAG0 = -(-TAIL // HOP)                         # a complete frame trails the newest sample by ceil(tail / hop) frames
WAYS = ("prompt", "lagged", "big", "bursts", "one")


def _session(rng, M, steps):
    """steps chunks of 6 samples (steps a multiple of 4, so chunks of 24 cut it too) -> (audio (M, S), labels (n,), best (n,))."""
    S = steps * 6
    n = max(0, (S - TAIL) // HOP)
    lab = np.zeros(n, np.uint8)
    t = int(rng.integers(0, 6))
    while t < n:
        run = int(rng.integers(1, 22))
        lab[t:t + run] = 1
        t += run + int(rng.integers(1, 14))
    best = np.repeat(rng.integers(0, M, n + 1), rng.integers(1, 5, n + 1))[:n].astype(np.uint8)     # runs of 1 .. 4 frames
    assert len(best) == n
    audio = rng.integers(-30000, 30000, (M, S)).astype(np.int16)
    return audio, lab, best


def _frontier(way, rng, S, n, chunk, lag):
    """The (labels, best bytes) received after every step, inside the preconditions: F >= floor(A / hop) - lag, F <= Fb <= floor(A / hop)."""
    out, F = [], 0
    steps = S // chunk
    for s in range(steps):
        A = (s + 1) * chunk
        Fb = min(n, max(0, (A - TAIL) // HOP))
        lo = min(Fb, max(F, A // HOP - lag, 0))
        F = Fb if way in ("prompt", "big", "one") else lo if way == "lagged" else int(rng.integers(lo, Fb + 1))
        assert A // HOP - lag <= F <= Fb <= A // HOP
        out.append((F, Fb))
    out[-1] = (n, n)
    return out


def _run(way, rng, cfg, M, D, audio, lab, best, extra_lag=5, hist=None, best_hist=None):
    S, n = audio.shape[1], len(lab)
    chunk = {"big": 24, "one": S}.get(way, 6)
    lag = LAG0 + (0 if way in ("prompt", "big", "one") else extra_lag)
    hist = gg.history(cfg, lag, chunk, D) if hist is None else hist
    best_hist = gg.best_history(cfg, lag, chunk, D) if best_hist is None else best_hist
    fr = _frontier(way, rng, S, n, chunk, lag)
    ld_lab = max(max(b[0] - a[0] for a, b in zip([(0, 0)] + fr, fr)), 1)
    ld_out, ms = gg.max_out(cfg, ld_lab, chunk, D), gg.max_seg(cfg, ld_lab)
    grp = gg.Group(cfg, M, hist, best_hist, D)
    res = gg.run_session(grp, audio, best, lab, chunk, fr, ld_out, ms)
    for out, seg, count in res:
        assert count <= ms and (seg["n_stored"] == seg["n"]).all()         # nothing truncated at the derived sizes
    return grp, res, (hist, best_hist, chunk, lag, [f for f, _ in fr])


CASES = [(M, pad, W, D) for M in (1, 2, 3) for pad in (0, 1, 5) for W in (0, 7) for D in (1, 3, 7, 1000)]


@pytest.fixture(scope="module")
def sweep():
    """Every (M, pad, max_len, D) x 4 random sessions x the five ways of cutting: run once, shared by the tests below."""
    rng = np.random.default_rng(20240607)
    runs = []
    for M, pad, W, D in CASES:
        cfg = (pad, W, 0, HOP, LEAD, TAIL)
        for _ in range(4):
            audio, lab, best = _session(rng, M, 4 * int(rng.integers(6, 20)))
            want = gg.offline(lab, best, audio, cfg, D)
            for way in WAYS:
                grp, res, sizes = _run(way, rng, cfg, M, D, audio, lab, best)
                runs.append((cfg, M, D, way, audio, lab, best, want, grp, res, sizes))
    return runs


def test_step_equals_offline_definition_however_the_session_is_cut(sweep):
    assert len(sweep) == len(CASES) * 4 * 5 and len(sweep) // 5 >= 200
    seen = set()
    for cfg, M, D, way, audio, lab, best, want, grp, res, sizes in sweep:
        got = gg.session_cuts(res)
        assert len(got) == len(want), (cfg, M, D, way)
        for (f, k, fl, data, done), (wf, wk, wp, wdata) in zip(got, want):
            assert (f, k, gg.channel(fl)) == (wf, wk, wp) and done, (cfg, M, D, way)
            assert not fl & (gg.LOST | gg.SHORT | gg.UNSYNC)
            assert data.dtype == wdata.dtype and data.tobytes() == wdata.tobytes(), (cfg, M, D, way, f)
        assert grp.voteless == 0                                            # every frame of every choice window was in the ring
        seen |= grp.trace
    assert {"deferred", "backlog", "closed below D", "split"} <= seen


def test_decide_at_least_max_len_is_the_table_pick_gather_chain(sweep):
    n = 0
    for cfg, M, D, way, audio, lab, best, want, grp, res, sizes in sweep:
        if not (cfg[1] > 0 and D >= cfg[1]):
            continue
        tab, _ = cuts_ref.table(lab[None, :], None, None, audio.shape[1], cfg)
        picked, picks = fuse_ref.pick_ref(best[None, :], [list(range(M))], [tuple(c) for c in tab.tolist()])
        ld = max([int(c["n_samples"]) for c in tab] + [1])
        ref, ref_len = cuts_ref.gather(audio, np.array(picked, cuts_ref.CUT_DTYPE), "samples", ld, np.zeros((len(tab), ld), np.int16),
                                       np.zeros(len(tab), np.int64))
        got = gg.session_cuts(res)
        assert len(got) == len(tab)
        for i, (f, k, fl, data, done) in enumerate(got):
            assert gg.channel(fl) == picks[i] and len(data) == ref_len[i] and data.tobytes() == ref[i, :ref_len[i]].tobytes()
        n += len(got)
    assert n > 500


def test_decide_1_defers_nothing_and_gives_the_mono_gates_records(sweep):
    n = 0
    for cfg, M, D, way, audio, lab, best, want, grp, res, (hist, bh, chunk, lag, fr) in sweep:
        if D != 1:
            continue
        assert hist == gr.history(cfg, lag, chunk) and "deferred" not in grp.trace
        mono = gr.Slot(cfg, hist)
        F0 = 0
        for s, (out, seg, count) in enumerate(res):
            fl = (gr.START if s == 0 else 0) | (gr.END if s == len(res) - 1 else 0)
            mout, mseg, mcount = mono.step(audio[0, s * chunk:(s + 1) * chunk], lab[F0:fr[s]], fl, len(out), len(seg) + 4)
            F0 = fr[s]
            assert count == mcount
            for name in gr.SEG_DTYPE.names:
                assert ((seg[name] & 0xff) if name == "flags" else seg[name]).tolist() == mseg[name].tolist(), name
            off = 0
            for r in seg:                                                   # each fragment: the mono gate's sample range of the chosen row
                src = max(int(r["first_frame"]) * HOP - LEAD, 0) + int(r["offset"])
                assert out[off:off + r["n"]].tobytes() == audio[gg.channel(r["flags"]), src:src + r["n"]].tobytes()
                off += int(r["n"])
            if M == 1:
                assert out.tobytes() == mout.tobytes()
            n += count
    assert n > 1000


def test_deepest_reads_against_the_bounds(sweep, capsys):
    """Under the preconditions the deepest PCM read stays inside uvad_gate_group_history and the deepest best read inside
    uvad_gate_group_best_history; how close they come is printed (DESIGN.md 3.23 quotes it)."""
    slack_pcm, slack_best = [], []
    for cfg, M, D, way, audio, lab, best, want, grp, res, (hist, bh, chunk, lag, fr) in sweep:
        if way == "one":
            continue                                                        # one step: the ring holds the whole session
        assert grp.deep_pcm <= hist and grp.deep_best <= bh, (cfg, D, way)
        if grp.deep_pcm:
            slack_pcm.append((hist - grp.deep_pcm, way, D))
            slack_best.append((bh - grp.deep_best, way, D))
    with capsys.disabled():
        print(f"\n  group gate: smallest slack of the PCM ring {min(slack_pcm)} samples, of the best ring {min(slack_best)} frames")
    assert min(slack_pcm)[0] >= 1 and min(slack_best)[0] >= 1               # the derivation leaves one place
    assert min(slack_pcm)[0] <= 2 * HOP and min(slack_best)[0] <= 3         # ... and the bounds are not loose: some session comes that close


def test_rings_below_the_bound_lose_samples_and_votes():
    rng = np.random.default_rng(5)
    cfg, M, D = (1, 0, 0, HOP, LEAD, TAIL), 2, 7
    lost = voteless = 0
    for _ in range(40):
        audio, lab, best = _session(rng, M, 40)
        lag = LAG0 + 5
        grp, res, _ = _run("lagged", rng, cfg, M, D, audio, lab, best, hist=gg.history(cfg, lag, 6, D) - 3 * HOP,
                           best_hist=gg.best_history(cfg, lag, 6, D) - 4)
        got = gg.session_cuts(res)
        want = gg.offline(lab, best, audio, cfg, D)
        assert [(f, k) for f, k, *_ in got] == [(f, k) for f, k, *_ in want]    # the cuts themselves do not depend on the rings
        for (f, k, fl, data, done), (wf, wk, wp, wdata) in zip(got, want):
            if fl & gg.LOST:
                lost += 1
                assert len(data) == len(wdata) and (data[:1] == 0).all()        # what has left the ring is zeros
            elif gg.channel(fl) == wp:
                assert data.tobytes() == wdata.tobytes()
        voteless += grp.voteless
    assert lost > 0 and voteless > 0


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------------
def _hand(lab, best, M, D, pad=0, W=0, chunk=6, way="prompt"):
    n = len(lab)
    S = -(-(n * HOP + TAIL) // 24) * 24
    n_all = (S - TAIL) // HOP
    lab = np.concatenate([np.asarray(lab, np.uint8), np.zeros(n_all - n, np.uint8)])
    best = np.concatenate([np.asarray(best, np.uint8), np.zeros(n_all - n, np.uint8)])
    audio = (np.arange(S)[None, :] % 997 + 1000 * (np.arange(M)[:, None] + 1)).astype(np.int16)
    cfg = (pad, W, 0, HOP, LEAD, TAIL)
    outs = []
    for way in WAYS:
        grp, res, _ = _run(way, np.random.default_rng(1), cfg, M, D, audio, lab, best)
        cuts = gg.session_cuts(res)
        want = gg.offline(lab, best, audio, cfg, D)
        assert [(f, k, gg.channel(fl), d.tobytes()) for f, k, fl, d, _ in cuts] == [(f, k, p, d.tobytes()) for f, k, p, d in want], way
        outs.append(([(f, k, gg.channel(fl)) for f, k, fl, d, _ in cuts], res, grp))
    assert all(o[0] == outs[0][0] for o in outs)
    return outs[0][0], outs


def test_hand_winner_of_the_first_frames_is_not_the_winner_of_the_cut():
    lab = [0, 0] + [1] * 10 + [0] * 4
    best = [0, 0] + [0] * 3 + [1] * 7 + [0] * 4
    assert _hand(lab, best, 2, 3)[0] == [(2, 10, 0)]                        # frames 2 .. 4 say 0
    assert _hand(lab, best, 2, 1000)[0] == [(2, 10, 1)]                     # the whole cut says 1: fuse_pick's answer
    assert _hand(lab, best, 2, 7)[0] == [(2, 10, 1)]                        # 3 against 4


def test_hand_vote_ties_go_to_the_lowest_position():
    lab = [0] + [1] * 6 + [0] * 3
    assert _hand(lab, [0, 1, 0, 1, 0, 1, 0, 0, 0, 0], 2, 6)[0] == [(1, 6, 0)]
    assert _hand(lab, [0, 2, 1, 2, 1, 2, 1, 0, 0, 0], 3, 6)[0] == [(1, 6, 1)]
    assert _hand(lab, [0, 2, 1, 0, 2, 1, 0, 0, 0, 0], 3, 6)[0] == [(1, 6, 0)]
    assert _hand(lab, [0, 7, 9, 7, 9, 200, 255, 0, 0, 0], 3, 6)[0] == [(1, 6, 0)]      # bytes at or above the group's size: no votes


def test_hand_a_piece_that_closes_below_the_horizon_chooses_on_what_it_has():
    lab = [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    best = [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    cuts, outs = _hand(lab, best, 2, 5)
    assert cuts == [(3, 2, 1)]
    for _, res, grp in outs:
        recs = np.concatenate([seg for _, seg, _ in res])
        assert len(recs) == 1 and recs[0]["flags"] & 0xff == gg.FIRST | gg.LAST          # nothing before the close, then everything
        assert "closed below D" in grp.trace


def test_hand_split_pieces_choose_for_themselves():
    lab = [0] + [1] * 8 + [0] * 3
    best = [0] + [0] * 4 + [1] * 4 + [0] * 3
    assert _hand(lab, best, 2, 4, W=4)[0] == [(1, 4, 0), (5, 4, 1)]
    assert _hand(lab, best, 2, 1, W=4)[0] == [(1, 4, 0), (5, 4, 1)]
    assert _hand(lab, [0, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0], 2, 1, W=4)[0] == [(1, 4, 1), (5, 4, 0)]   # D = 1: the first frame alone


def test_hand_an_interval_that_ends_on_a_piece_boundary_leaves_no_empty_piece():
    lab = [0] + [1] * 8 + [0] * 5
    cuts, outs = _hand(lab, [1] * 14, 2, 4, W=4)
    assert cuts == [(1, 4, 1), (5, 4, 1)]
    cuts, _ = _hand(lab, [1] * 14, 2, 4, pad=1, W=5)                        # [0, 10): two full pieces, with the pad
    assert cuts == [(0, 5, 1), (5, 5, 1)]


def test_unsync_marks_every_record_from_the_step_to_the_end():
    cfg = (0, 0, 0, HOP, LEAD, TAIL)
    rng = np.random.default_rng(3)
    audio, lab, best = _session(rng, 2, 40)
    lab[:] = 0
    lab[2:50] = 1
    S, n = audio.shape[1], len(lab)
    fr = _frontier("prompt", rng, S, n, 6, LAG0)
    grp = gg.Group(cfg, 2, gg.history(cfg, LAG0, 6, 3), gg.best_history(cfg, LAG0, 6, 3), 3)
    res = gg.run_session(grp, audio, best, lab, 6, fr, 400, 8, differ={10})
    flags = [[int(f) for f in seg["flags"]] for _, seg, _ in res]
    assert all(not f & gg.UNSYNC for fs in flags[:10] for f in fs) and any(flags[:10])
    assert all(f & gg.UNSYNC for fs in flags[10:] for f in fs) and sum(len(fs) for fs in flags[10:]) > 5
    res = gg.run_session(grp, audio, best, lab, 6, fr, 400, 8)               # the next session starts clean
    assert all(not f & gg.UNSYNC for _, seg, _ in res for f in seg["flags"])
