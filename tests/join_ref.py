"""A numpy restatement of the cut-supervision join (uvad_cuts_join, include/uvad.h), written from the header's definitions alone: a
brute-force double loop over a cut table and item lists, nothing shared with the kernels' searches, ballots or prefixes.  The GPU tests
compare bytes with it; tests/test_join_ref.py compares it with a transcription of the reference's loop and with hand-made answers."""
import numpy as np

from cuts_ref import CUT_DTYPE

OVERLAP, INSIDE = 0, 1
AUDIT_WORDS = 8
ITEMS, CUTS, PAIRS, MATCHED, UNMATCHED, EXCEEDING, REPEATED, EMPTY = range(AUDIT_WORDS)      # the words of one audit row


def matches(mode, f, k, s, e):
    """Does the item [s, e) match the cut [f, f + k)?"""
    if e <= s:
        return False
    if mode == OVERLAP:
        return s < f + k and e > f
    if mode == INSIDE:
        return s >= f and e <= f + k
    raise ValueError(f"unknown mode {mode!r}")


def exceeds(f, k, s, e):
    return f > s or f + k < e


def join(table, row_first, items, counts, mode, max_cuts=None, max_pairs=None, item_cuts=None):
    """table: CUT_DTYPE array and row_first (B + 1,) as cuts_ref.table returns them (the WHOLE table: max_cuts truncates here, as the
    device's table is truncated); items (B, max_iv, 2) int {s, e}; counts (B,) (clamped to [0, max_iv]).
    -> dict: per_cut (list over the m cuts taking part of lists of item indices), pair_first (m + 1,) int32, pairs (all of them, int32),
    stored (pairs[:max_pairs]), item_cuts (B, max_iv, 2) int32 -- the array passed in (default: filled with -7) with the slots below each
    row's count overwritten --, audit (B + 1, 8) uint64."""
    table = np.asarray(table, dtype=CUT_DTYPE)
    items = np.asarray(items).reshape(len(counts), -1, 2)
    B, max_iv = items.shape[0], items.shape[1]
    if mode not in (OVERLAP, INSIDE):
        raise ValueError(f"unknown mode {mode!r}")
    m = len(table) if max_cuts is None else min(len(table), int(max_cuts))
    out_items = np.full((B, max_iv, 2), -7, np.int32) if item_cuts is None else item_cuts
    audit = np.zeros((B + 1, AUDIT_WORDS), np.uint64)
    per_cut = []
    for b in range(B):
        nb = min(max(int(counts[b]), 0), max_iv)
        c0, c1 = min(int(row_first[b]), m), min(int(row_first[b + 1]), m)
        row = [[] for _ in range(c0, c1)]
        n_of = [0] * nb
        first_of = [-1] * nb
        exceeding = 0
        s, e = items[b, :nb, 0].astype(np.int64), items[b, :nb, 1].astype(np.int64)
        for i in range(c0, c1):                                          # every cut against every item of its row (the inner loop is numpy's)
            f, k = int(table[i]["first_frame"]), int(table[i]["n_frames"])
            assert int(table[i]["row"]) == b
            hit = (e > s) & ((s < f + k) & (e > f) if mode == OVERLAP else (s >= f) & (e <= f + k))
            assert all(matches(mode, f, k, int(s[j]), int(e[j])) for j in np.flatnonzero(hit)[:4])
            for j in np.flatnonzero(hit).tolist():
                row[i - c0].append(j)
                if n_of[j] == 0:
                    first_of[j] = i
                assert first_of[j] + n_of[j] == i                     # an item's cuts are a run
                n_of[j] += 1
                exceeding += exceeds(f, k, int(s[j]), int(e[j]))
        for j in range(nb):
            out_items[b, j] = first_of[j], n_of[j]
        pairs = sum(n_of)
        matched = sum(1 for n in n_of if n)
        audit[b] = nb, c1 - c0, pairs, matched, nb - matched, exceeding, pairs - matched, sum(1 for r in row if not r)
        per_cut += row
    audit[B] = audit[:B].sum(axis=0)
    pair_first = np.zeros(m + 1, np.int32)
    pair_first[1:] = np.cumsum([len(r) for r in per_cut])
    pairs = np.asarray([j for r in per_cut for j in r], np.int32).reshape(-1)
    stored = pairs if max_pairs is None else pairs[:max(int(max_pairs), 0)]
    return {"per_cut": per_cut, "pair_first": pair_first, "pairs": pairs, "stored": stored, "item_cuts": out_items, "audit": audit, "m": m}


def interesting(res):
    """The condition a seeded case must meet to prove anything: at least one pair, one repeated pair, one exceeding pair, one unmatched
    item and one empty cut in the pooled audit."""
    a = res["audit"][-1]
    return bool(a[PAIRS] > 0 and a[REPEATED] > 0 and a[EXCEEDING] > 0 and a[UNMATCHED] > 0 and a[EMPTY] > 0)
