"""CPU checks of the numpy restatement of the cut-supervision join (tests/join_ref.py, the yardstick of tests/test_gpu_join.py) against
a literal transcription of the reference's loop over new cuts and their supervisions (src/scripts/predict.py:513-586, the counters of
:525-541 with their round(., 2), the report's arithmetic of :595-609) in seconds on a 10 ms grid, against hand-made answers at every
border of the two match rules, and of the host helpers read_supervisions, cut_transcripts and join_report."""
import numpy as np
import pytest

import cuts_ref as cr
import join_ref as jr

SHIFT = 0.01


def reference_loop(windows_s, sups_s, words=False):
    """The reference's loop for one recording.  windows_s: [(abs_start, abs_end)] seconds, the new cuts; sups_s: [(start, duration)].
    Every time is compared after round(., 2), as the reference's own counter updates do (:530-535): on a 10 ms grid that is the same
    double for the same frame however it was computed (start + duration is not).  truncate(keep_excessive_supervisions=True) keeps the
    supervisions [s, e) with s < abs_end and e > abs_start; words=True is the rule of :565-568 instead.
    -> (supervision indices per cut, the seven counters in the report's order)."""
    sup_dict, sup_set = {}, set()
    empty_cut, in_sup, exceed_sup, in_multiple_sup = 0, 0, 0, 0
    for j, (start, duration) in enumerate(sups_s):
        sup_dict[j] = [start, duration, None, 0]
    per_cut = []
    for abs_start, abs_end in windows_s:
        cut_start, cut_end = round(abs_start, 2), round(abs_end, 2)
        new_sups = []
        for j, (start, duration) in enumerate(sups_s):
            sup_start, sup_end = round(start, 2), round(start + duration, 2)
            if not sup_end > sup_start:
                continue                                                      # an empty supervision is in no interval tree
            if words:
                if sup_start >= cut_start and sup_end <= cut_end:
                    new_sups.append(j)
            elif sup_start < cut_end and sup_end > cut_start:
                new_sups.append(j)
        if len(new_sups) != 0:
            for j in new_sups:
                in_sup += 1
                sup_set.add(j)
                sup_dict[j][3] += 1
                sup_start, sup_end = round(sup_dict[j][0], 2), round(sup_dict[j][0] + sup_dict[j][1], 2)
                if cut_start > sup_start or cut_end < sup_end:
                    exceed_sup += 1
                if sup_dict[j][3] > 1:
                    in_multiple_sup += 1
        else:
            empty_cut += 1
        per_cut.append(new_sups)
    not_in_sup = len(sup_dict.keys()) - len(sup_set)
    return per_cut, [len(sup_dict.keys()), in_sup, len(sup_set), not_in_sup, exceed_sup, in_multiple_sup, empty_cut]


REPORT_WORDS = [jr.ITEMS, jr.PAIRS, jr.MATCHED, jr.UNMATCHED, jr.EXCEEDING, jr.REPEATED, jr.EMPTY]


def seeded_items(rng, B, max_iv, counts, T):
    """Unsorted, overlapping items: most short and inside the row, some long, some empty or reversed, some outside the row."""
    iv = np.zeros((B, max_iv, 2), np.int32)
    for b in range(B):
        for j in range(max_iv):
            kind = rng.integers(0, 10)
            s = int(rng.integers(-5, T + 5))
            n = int(rng.integers(1, 12)) if kind < 6 else int(rng.integers(12, max(T // 2, 14))) if kind < 8 else int(rng.integers(-3, 1))
            if kind == 9:
                s = int(rng.choice([-40, T + 3]))
                n = int(rng.integers(1, 20))
            iv[b, j] = s, s + n
    return iv, np.asarray(counts, np.int32)


@pytest.mark.parametrize("mode", [jr.OVERLAP, jr.INSIDE])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_equals_the_reference_loop(mode, seed):
    rng = np.random.default_rng(seed)
    B, T, max_iv = 4, 400, 30
    labels = (np.cumsum(rng.random((B, T)) < 0.06, axis=1) % 2).astype(np.uint8)
    lens = [T, 311, 0, T - 1]
    table, first = cr.table(labels, lens, None, T * 160 + 240, (3, 25, 2, 160, 0, 240))
    iv, counts = seeded_items(rng, B, max_iv, [30, 17, 9, 30], T)
    res = jr.join(table, first, iv, counts, mode)
    assert jr.interesting(res) or mode == jr.INSIDE
    assert res["audit"][-1][jr.PAIRS] > 0 and res["audit"][-1][jr.UNMATCHED] > 0 and res["audit"][-1][jr.EMPTY] > 0
    for b in range(B):
        rows = table[first[b]:first[b + 1]]
        windows = [(int(c["first_frame"]) * SHIFT, (int(c["first_frame"]) + int(c["n_frames"])) * SHIFT) for c in rows]
        sups = [(int(s) * SHIFT, int(e) * SHIFT - int(s) * SHIFT) for s, e in iv[b, :counts[b]]]
        per_cut, counters = reference_loop(windows, sups, words=mode == jr.INSIDE)
        assert per_cut == res["per_cut"][first[b]:first[b + 1]]
        assert counters == [int(res["audit"][b][w]) for w in REPORT_WORDS], (b, counters, res["audit"][b])
        assert int(res["audit"][b][jr.CUTS]) == len(rows)
    assert np.array_equal(res["audit"][-1], res["audit"][:-1].sum(axis=0))
    assert int(res["audit"][-1][jr.PAIRS]) == int(res["item_cuts"][:, :, 1][res["item_cuts"][:, :, 1] > 0].sum()) == len(res["pairs"])


def hand_table(rows):
    """rows: per row a list of (first_frame, n_frames) -> (CUT_DTYPE table, row_first)."""
    out, first = [], [0]
    for b, cuts in enumerate(rows):
        out += [(b, k, f, n, f * 160, n * 160) for k, (f, n) in enumerate(cuts)]
        first.append(len(out))
    return np.array(out, dtype=cr.CUT_DTYPE).reshape(-1), np.asarray(first, np.int32)


# one row of 200 frames; the cuts [10, 20) [20, 30) (two adjacent split pieces) and [40, 50)
HAND_CUTS = [[(10, 10), (20, 10), (40, 10)]]
HAND = [  # (item, cuts matched by OVERLAP, exceeding pairs, cuts matched by INSIDE)
    ((0, 10), [], 0, []),             # ends exactly at f
    ((30, 40), [], 0, []),            # starts exactly at f + k of one cut and ends exactly at f of the next
    ((0, 11), [0], 1, []),            # the same moved by one frame
    ((29, 40), [1], 1, []),
    ((30, 41), [2], 1, []),
    ((50, 60), [], 0, []),            # starts exactly at f + k
    ((49, 60), [2], 1, []),
    ((40, 50), [2], 0, [2]),          # equal to a cut
    ((41, 49), [2], 0, [2]),
    ((40, 51), [2], 1, []),
    ((39, 50), [2], 1, []),
    ((15, 25), [0, 1], 2, []),        # across the border of two adjacent pieces
    ((10, 30), [0, 1], 2, []),
    ((10, 20), [0], 0, [0]),
    ((20, 30), [1], 0, [1]),
    ((19, 21), [0, 1], 2, []),
    ((5, 100), [0, 1, 2], 3, []),
    ((25, 25), [], 0, []),            # e <= s
    ((25, 15), [], 0, []),
    ((45, 44), [], 0, []),
    ((-30, 11), [0], 1, []),          # negative s
    ((-30, -10), [], 0, []),
    ((-5, 0), [], 0, []),
    ((45, 1000), [2], 1, []),         # e past the row
    ((-(1 << 31), (1 << 31) - 1), [0, 1, 2], 3, []),
    ((300, 400), [], 0, []),
]


@pytest.mark.parametrize("mode", [jr.OVERLAP, jr.INSIDE])
def test_hand_made_answers(mode):
    table, first = hand_table(HAND_CUTS)
    iv = np.asarray([[it for it, _, _, _ in HAND]], np.int64).astype(np.int32)
    res = jr.join(table, first, iv, [len(HAND)], mode)
    want_cuts = [h[1] if mode == jr.OVERLAP else h[3] for h in HAND]
    assert res["item_cuts"][0].tolist() == [[c[0], len(c)] if c else [-1, 0] for c in want_cuts]
    assert res["per_cut"] == [[j for j, c in enumerate(want_cuts) if i in c] for i in range(3)]
    pairs = sum(len(c) for c in want_cuts)
    matched = sum(1 for c in want_cuts if c)
    exceeding = sum(h[2] for h in HAND) if mode == jr.OVERLAP else 0
    assert res["audit"][0].tolist() == [len(HAND), 3, pairs, matched, len(HAND) - matched, exceeding, pairs - matched, 0]
    assert res["pair_first"].tolist() == np.concatenate(([0], np.cumsum([len(r) for r in res["per_cut"]]))).tolist()
    assert res["pairs"].tolist() == [j for r in res["per_cut"] for j in r]
    if mode == jr.OVERLAP:
        assert (pairs, matched, exceeding) == (24, 17, 20)
    else:
        assert (pairs, matched) == (4, 4)


def test_truncation_empty_rows_and_untouched_slots():
    table, first = hand_table([[(0, 5), (10, 5)], [], [(3, 4)], [(0, 2), (2, 2), (4, 2)]])
    iv = np.zeros((4, 3, 2), np.int32)
    iv[0] = [[4, 11], [20, 30], [0, 0]]
    iv[1] = [[0, 100], [0, 100], [0, 100]]         # a row without cuts: its items are counted, none is matched
    iv[2] = [[3, 7], [0, 100], [5, 6]]
    iv[3] = [[0, 6], [1, 3], [9, 9]]
    counts = [3, 2, 7, -4]                         # clamped to [0, max_iv]
    full = jr.join(table, first, iv, counts, jr.OVERLAP)
    assert full["per_cut"] == [[0], [0], [0, 1, 2], [], [], []]
    assert full["audit"].tolist() == [[3, 2, 2, 1, 2, 2, 1, 0], [2, 0, 0, 0, 2, 0, 0, 0], [3, 1, 3, 3, 0, 1, 0, 0], [0, 3, 0, 0, 0, 0, 0, 3],
                                      [8, 6, 5, 4, 4, 3, 1, 3]]
    assert full["item_cuts"][1].tolist() == [[-1, 0], [-1, 0], [-7, -7]] and (full["item_cuts"][3] == -7).all()
    assert full["item_cuts"][0].tolist() == [[0, 2], [-1, 0], [-1, 0]] and full["item_cuts"][2].tolist() == [[2, 1], [2, 1], [2, 1]]
    cut = jr.join(table, first, iv, counts, jr.OVERLAP, max_cuts=1, max_pairs=0)      # only the first cut takes part
    assert cut["m"] == 1 and cut["per_cut"] == [[0]] and cut["pair_first"].tolist() == [0, 1] and len(cut["stored"]) == 0 and len(cut["pairs"]) == 1
    assert cut["audit"].tolist() == [[3, 1, 1, 1, 2, 1, 0, 0], [2, 0, 0, 0, 2, 0, 0, 0], [3, 0, 0, 0, 3, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0],
                                     [8, 1, 1, 1, 7, 1, 0, 0]]
    some = jr.join(table, first, iv, counts, jr.OVERLAP, max_pairs=3)
    assert some["stored"].tolist() == [0, 0, 0] and some["pairs"].tolist() == [0, 0, 0, 1, 2] and np.array_equal(some["audit"], full["audit"])
    inside = jr.join(table, first, iv, counts, jr.INSIDE)
    assert inside["per_cut"] == [[], [], [0, 2], [], [], []] and inside["audit"][-1].tolist() == [8, 6, 2, 2, 6, 0, 0, 5]
    assert not jr.interesting(inside) and jr.interesting(full)


def test_read_supervisions_and_transcripts(tmp_path):
    from uvad_amd.postprocess import cut_transcripts, read_label_file, read_supervisions
    p = tmp_path / "sup.txt"
    p.write_text("0.50\t1.25\thello there\n\n1.25\t2.0\tgeneral  kenobi \n2.5\t3.0\n3.0\t3.5\tyou\tare\n")
    sups = read_supervisions(str(p))
    assert sups == [(0.5, 1.25, "hello there"), (1.25, 2.0, "general  kenobi"), (2.5, 3.0, None), (3.0, 3.5, "you\tare")]
    assert read_label_file(str(p)) == [(s, e) for s, e, _ in sups]                      # the older reader sees the same intervals
    (tmp_path / "bad.txt").write_text("0.5\n")
    with pytest.raises(ValueError):
        read_supervisions(str(tmp_path / "bad.txt"))
    texts = [t for _, _, t in sups]
    assert cut_transcripts([[0, 1], [], [2], [1, 2, 3], [3, 0]], texts) == ["hello there general  kenobi", "", "", "general  kenobi you\tare", "you\tare hello there"]
    assert cut_transcripts([[0, 1]], [" a ", "b "]) == ["a  b"]                         # text + " " per item, stripped at the ends only


def test_join_report_is_the_reference_block():
    from uvad_amd.postprocess import JOIN_REPORT_NAMES, join_report
    counters = [12, 9, 7, 5, 4, 2, 3]
    audit = dict(zip(JOIN_REPORT_NAMES, counters))
    text = join_report({"rows": [], "pooled": {**audit, "New cuts": 8}}, "ami", 0.1, "test")
    assert text == ("Dataset: ami, Buffer: 0.1, Phase: test\n\n----------------\nTotal Supervisions: 12\nSupervisions in new cuts: 9\n"
                    "Unique Supervisions in new cuts: 7\nSupervisions not in new cuts: 5\nSupervisions exceeding new cuts: 4\n"
                    "Supervisions in multiple new cuts: 2\nEmpty cuts: 3\n")
    assert join_report(audit, "ami", 0.1, "test") == text
