"""The step rule of the live speech gate (tests/gate_ref.py) against the offline pair it is the streaming counterpart of: for random
sessions, however their samples and labels are cut into steps, the fragments a slot emits, concatenated per cut, are the bytes, first
frames, frame counts and indices of tests/cuts_ref.py's table + gather on the whole session; with max_len = 0 the cut boundaries are the
median endpointer's event frames (tests/endpoint_ref.py).  build() below also makes the step inputs of the GPU tests."""
import numpy as np
import pytest

import cuts_ref as cr
import endpoint_ref as er
import gate_ref as gr

LD_LAB = 125
FRAME = {4: (3, 3), 160: (120, 120)}          # hop -> the natural (lead, tail): frame_len 10 at hop 4, 400 at hop 160
SCHEDULES = {                                  # name -> (chunk in half hops, label lag in frames)
    "prompt": (2, 0),                          # one hop per step, a label the moment its frame is complete: one label per step
    "late": (3, 9),                            # a hop and a half per step (every other chunk starts inside a frame), labels 9 frames late
    "at_end": (4, 135),                        # every label in the END step
    "bursts": (6, 6),                          # a random number of the complete frames' labels, at most 6 held back
    "big": (12, 0),                            # large steps: many labels at once
}
BASE = 12                                      # half hops: every chunk size divides it, so one session can be cut at every schedule
CONFIGS = [(pad, max_len, 0, hop) + lt for hop in (4, 160) for pad in (0, 2, 5) for max_len in (0, 1, 7) for lt in (FRAME[hop], (0, 0))]
WANTED = {"split", "rejoin", "ended open", "ended pending", "one-step session", "restart without END", "empty piece", "ring wrap"}


def random_labels(rng, n):
    """n labels in runs and gaps of 1 .. 9 frames, a non-zero byte for speech."""
    out, v = [], int(rng.integers(0, 2))
    while len(out) < n:
        out += [v * int(rng.choice([1, 255]))] * int(rng.integers(1, 10))
        v ^= 1
    return np.asarray(out[:n], np.uint8)


def schedule_lag(sched, hop):
    """The lag_frames the schedule keeps: the label frontier trails floor(samples / hop) by its own lag and by the frame's tail."""
    return SCHEDULES[sched][1] + -(-FRAME[hop][1] // hop)


def build(cfg, sched, seed, B=3, per_slot=12, dtype=np.int16, max_frames=108, chunk=None):
    """Step inputs for B slots, each hosting per_slot sessions one after another -> dict(chunks (steps, B, q), labels (steps, B, LD_LAB),
    lab_counts, flags, q, sessions = [dict(b, s0, s1, ended, labels, pcm, kind)], live (steps, B)).  A session's labels and PCM depend on
    (seed, slot, number) alone and its length is a multiple of BASE half hops, so every schedule cuts the very same sessions (but the
    one-step ones, which are one chunk long); the schedule decides the chunk size and when a label arrives: frame t is complete, and
    its label available, once (t + 1) hop + the natural tail samples have arrived, and the END step hands over every label that is
    left.  Kinds: whole sessions, sessions whose audio stops at half their labels (pieces with empty sample ranges), sessions abandoned
    by the next START, sessions of one step.  Idle rows, label columns past the count and the counts of idle slots hold junk.
    chunk: samples per step instead of the schedule's own (sessions are then multiples of it)."""
    pad, max_len, _, hop, lead, tail = cfg
    rng = np.random.default_rng([seed, 1 << 20])                            # timing alone: idle gaps, bursts, junk
    half, lag = SCHEDULES[sched]
    q, base, tail_nat = chunk or half * hop // 2, chunk or BASE * hop // 2, FRAME[hop][1]
    rows, sessions = [], []
    for b in range(B):
        steps = []                                                          # (chunk or None, labels, flag)
        for k in range(per_slot):
            kind = ("whole", "whole", "cut", "abandoned", "one")[k % 5]
            srng = np.random.default_rng([seed, b, k])                      # the session itself
            n = int(srng.integers(0, max_frames + 1)) if kind != "one" else 0
            gen = random_labels(srng, n + 16)
            if kind == "cut":
                S = max(1, -(-(n // 2) * hop // base)) * base
            elif kind == "one":
                S = q
            else:
                S = -(-(n * hop + tail_nat + 1) // base) * base
                n = max((S - tail_nat) // hop, 0)
            lab, ns = gen[:n], S // q
            pcm = (srng.integers(1, 30000, S + base) if np.dtype(dtype).kind == "i" else srng.uniform(0.1, 1.0, S + base)).astype(dtype)[:S]
            if kind == "abandoned":
                ns = max(1, ns // 2)
            s0, d = len(steps), 0
            for s in range(ns):
                avail = min(max(((s + 1) * q - tail_nat) // hop, 0), n)
                want = max(avail - lag, 0) if sched != "bursts" else max(avail - int(rng.integers(0, 7)), 0)
                last = s == ns - 1 and kind != "abandoned"
                d1 = n if last else max(d, want)
                steps.append((pcm[s * q:(s + 1) * q], lab[d:d1], (gr.START if s == 0 else 0) | (gr.END if last else 0)))
                d = d1
            sessions.append(dict(b=b, s0=s0, s1=len(steps) - 1, ended=kind != "abandoned", labels=lab, pcm=pcm, kind=kind))
            if kind != "abandoned":
                steps += [(None, None, 0)] * int(rng.integers(0, 3))        # idle steps; an abandoned session is cut off by the next START
        rows.append(steps)
    n_steps = max(len(r) for r in rows)
    junk = rng.integers(1, 30000, (n_steps, B, q))
    chunks = junk.astype(dtype) if np.dtype(dtype).kind == "i" else np.full((n_steps, B, q), np.nan, dtype)
    labels = np.full((n_steps, B, LD_LAB), 255, np.uint8)
    counts = rng.integers(-3, 9, (n_steps, B)).astype(np.int32)             # an idle slot's count is junk too
    flags = np.zeros((n_steps, B), np.uint8)
    for b, steps in enumerate(rows):
        for s, (c, lab, fl) in enumerate(steps):
            if c is not None:
                chunks[s, b], counts[s, b], flags[s, b] = c, len(lab), fl
                labels[s, b, :len(lab)] = lab
    live = np.zeros((n_steps, B), bool)
    for i, sess in enumerate(sessions):                                     # an abandoned session lives on until the slot's next START
        nxt = sessions[i + 1]["s0"] if i + 1 < len(sessions) and sessions[i + 1]["b"] == sess["b"] else n_steps
        live[sess["s0"]:(sess["s1"] + 1 if sess["ended"] else nxt), sess["b"]] = True
    return dict(chunks=chunks, labels=labels, lab_counts=counts, flags=flags, q=q, sessions=sessions, live=live)


def session_records(res, data, sess):
    """[(record, its samples)] a session's slot emitted over the session's steps."""
    out = []
    for s in range(sess["s0"], sess["s1"] + 1):
        row, seg, count = res[s][sess["b"]]
        assert count == len(seg), "max_seg was meant to suffice"
        off = 0
        for r in seg:
            out.append((r, row[off:off + int(r["n_stored"])]))
            off += int(r["n_stored"])
    return out


def check_session(cfg, sess, recs):
    """The fragments against cuts_ref on the whole session: every cut's index, first frame, frame count and bytes."""
    lab, pcm = sess["labels"], sess["pcm"]
    pad, max_len, min_len, hop, lead, tail = cfg
    cuts = gr.assemble(recs)
    if not sess["ended"]:                                                   # an abandoned session: what it did deliver sits where it says
        for r, data in recs:
            first = max(int(r["first_frame"]) * hop - lead, 0) + int(r["offset"])
            assert r["n"] == r["n_stored"] and np.array_equal(data, pcm[first:first + len(data)])
        return 0
    tab, _ = cr.table(lab[None, :] if len(lab) else np.zeros((1, 1), np.uint8), [len(lab)], [len(pcm)], len(pcm), cfg)
    assert len(cuts) == len(tab), (len(cuts), len(tab))
    ld = max(int(tab["n_samples"].max()), 1) if len(tab) else 1
    want, want_len = cr.gather(pcm[None, :], tab, "samples", ld, np.zeros((len(tab), ld), pcm.dtype), np.zeros(len(tab), np.int32))
    for i, (f, k, fl, samples, done) in enumerate(cuts):
        assert done and tab["index"][i] == i and (f, k) == (tab["first_frame"][i], tab["n_frames"][i]), (i, f, k, tab[i])
        assert not fl & (gr.LOST | gr.SHORT), (i, fl)
        assert len(samples) == want_len[i] == tab["n_samples"][i] and samples.tobytes() == want[i, :len(samples)].tobytes(), i
    if max_len == 0:                                                        # the median endpointer's events are the cut boundaries
        _, iv = er.whole((lab != 0).astype(np.float32), 1, pad)
        assert er.events_of(iv) == [e for f, k, *_ in cuts for e in ((er.START, f), (er.END, f + k))]
    return len(cuts)


def run(cfg, sched, seed, **kw):
    data = build(cfg, sched, seed, **kw)
    hop = cfg[3]
    H = gr.history(cfg, schedule_lag(sched, hop), data["q"])
    res, slots = gr.simulate(cfg, H, data["chunks"], data["labels"], data["lab_counts"], data["flags"],
                             gr.max_out(cfg, LD_LAB, data["q"]), gr.max_seg(cfg, LD_LAB))
    return data, res, slots


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_fragments_equal_the_offline_cuts_on_the_whole_session(sched):
    seen, n_cuts, n_sessions = set(), 0, 0
    for i, cfg in enumerate(CONFIGS):
        big = cfg[3] == 160
        data, res, slots = run(cfg, sched, 100 + i, B=2 if big else 3, per_slot=5 if big else 12)
        claimed = set()
        for sess in data["sessions"]:
            claimed |= set(range(sess["s0"], sess["s1"] + 1)) if sess["b"] == 0 else set()
            n_cuts += check_session(cfg, sess, session_records(res, data, sess))
            n_sessions += 1
        for s in range(data["flags"].shape[0]):                             # an idle slot emits nothing
            if s not in claimed:
                assert res[s][0][2] == 0
        for sl in slots:
            seen |= sl.trace
    print(f"{sched}: {n_sessions} sessions, {n_cuts} cuts, met {sorted(seen)}")
    assert n_cuts > 500
    assert WANTED <= seen, sorted(WANTED - seen)                            # the self-check: this schedule met every situation


def test_every_schedule_cuts_the_same_sessions():
    """Each session is cut at every one of the five schedules: same labels, same PCM, five sequences of steps."""
    for cfg in (CONFIGS[0], CONFIGS[-1]):
        runs = {sched: build(cfg, sched, 3)["sessions"] for sched in SCHEDULES}
        steps = set()
        for i, base in enumerate(runs["prompt"]):
            for sched, sessions in runs.items():
                assert sessions[i]["kind"] == base["kind"] and sessions[i]["labels"].tobytes() == base["labels"].tobytes()
                assert base["kind"] == "one" or sessions[i]["pcm"].tobytes() == base["pcm"].tobytes()
            if base["kind"] == "whole" and len(base["labels"]) > 20:
                steps.add(len({sessions[i]["s1"] - sessions[i]["s0"] for sessions in runs.values()}))
        assert steps == {5}                                                 # five different numbers of steps for one session


def test_one_label_per_step_and_everything_at_end_are_what_they_say():
    cfg = (2, 7, 0, 4, 3, 3)
    d = build(cfg, "prompt", 1)
    for sess in d["sessions"]:
        c = d["lab_counts"][sess["s0"]:sess["s1"], sess["b"]]               # every step but the END step
        assert c.max(initial=0) <= 1
    d = build(cfg, "at_end", 1)
    for sess in d["sessions"]:
        assert not d["lab_counts"][sess["s0"]:sess["s1"], sess["b"]].any()
        if sess["ended"]:
            assert d["lab_counts"][sess["s1"], sess["b"]] == len(sess["labels"])
    d = build(cfg, "late", 1)
    for sess in d["sessions"]:
        for s in range(sess["s0"], sess["s1"]):
            seen_labels = int(d["lab_counts"][sess["s0"]:s + 1, sess["b"]].sum())
            complete = max(((s - sess["s0"] + 1) * d["q"] - 3) // 4, 0)
            assert seen_labels <= max(complete - 9, 0)


def test_short_and_lost_are_flagged_where_the_header_says():
    """An oversize tail closes pieces before their samples are there (SHORT, and the cut is shorter than the offline one); a ring of
    chunk + hop samples loses the start of every padded piece (LOST, zero bytes)."""
    cfg = (2, 7, 0, 4, 3, 40)
    data, res, slots = run(cfg, "prompt", 5)
    flags = 0
    for sess in data["sessions"]:
        for r, _ in session_records(res, data, sess):
            flags |= int(r["flags"])
    assert flags & gr.SHORT and not flags & gr.LOST
    cfg = (5, 0, 0, 4, 3, 3)
    data = build(cfg, "late", 6)
    res, _ = gr.simulate(cfg, data["q"] + 4, data["chunks"], data["labels"], data["lab_counts"], data["flags"], gr.max_out(cfg, LD_LAB, data["q"]),
                         gr.max_seg(cfg, LD_LAB))
    lost = 0
    for sess in data["sessions"]:
        for r, samples in session_records(res, data, sess):
            if r["flags"] & gr.LOST:
                lost += 1
                assert samples[0] == 0                                      # the fragment's first sample has left the ring
    assert lost > 0


def test_bounds_hold_and_history_is_tight_enough():
    """max_seg and max_out were never exceeded above (session_records asserts it).  At gr.history's size nothing is lost on the worst
    schedule -- labels after the full lag, pad 5 -- nor with large chunks, where the deepest read lies beyond what a count without the
    chunk term, (lag + pad + 2) hop + lead, would keep."""
    cfg = (5, 7, 0, 4, 3, 3)
    for sched in ("late", "big"):
        data = build(cfg, sched, 7)
        lag = schedule_lag(sched, 4)
        H = gr.history(cfg, lag, data["q"])
        res, _ = gr.simulate(cfg, H, data["chunks"], data["labels"], data["lab_counts"], data["flags"], gr.max_out(cfg, LD_LAB, data["q"]),
                             gr.max_seg(cfg, LD_LAB))
        reach = 0
        for sess in data["sessions"]:
            A = 0
            for s in range(sess["s0"], sess["s1"] + 1):
                A += data["q"]
                for r in res[s][sess["b"]][1]:
                    assert not r["flags"] & gr.LOST
                    if r["n"]:
                        reach = max(reach, A - (max(int(r["first_frame"]) * 4 - 3, 0) + int(r["offset"])))
        print(f"{sched}: chunk {data['q']}, lag {lag}, history {H}, deepest read {reach}")
        assert reach <= H
        if sched == "big":
            assert reach > (lag + 5 + 2) * 4 + 3
