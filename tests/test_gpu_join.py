"""The cut-supervision join on the device (uvad_cuts_join, include/uvad.h) against the brute-force restatement tests/join_ref.py, byte for
byte, with labels -> uvad_cuts_table -> uvad_cuts_join on the device: a sweep of small shapes in both modes, the borders of the two match
rules on ballot-word boundaries, many cuts in one row, many rows, a long row, truncation by max_pairs and max_cuts, a NULL d_item_cuts,
determinism, one captured graph of table + join + gather replayed with new inputs, the host layer and predict_vad(supervisions=...).

EVERY comparison below (_check) runs with what must never be read poisoned -- item slots at or past a row's count hold {INT32_MIN,
INT32_MAX}, which would match every cut; so do all item slots of a row without cuts; table entries at or past the cuts taking part
hold a cut that covers every frame of row 0 -- and with every output pre-filled with a canary that must survive wherever the header says
"not written".  Every comparison also asserts, on the device's outputs alone, that the two sides of the audit agree: [2] equals the sum
of n over d_item_cuts, [4] = [0] - [3], [6] = [2] - [3], row B the column sums.

A randomized case proves nothing if its answer is empty: every seeded case asserts that the RESTATEMENT's answer holds at least one
pair, one unmatched item and one empty cut, and in OVERLAP mode one repeated and one exceeding pair (INSIDE can have neither: a word lies
whole inside at most one cut and never exceeds it).  The seeds were chosen on the CPU for that.  Exempt are the shapes that are in the
sweep for their own sake and cannot meet it by counting: T = 1 (a row has one cut at most), fewer than two items per row, length sets
of 0 and 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuts_ref as cr
import join_ref as jr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY = 0x5A
CANARY32 = int(np.frombuffer(bytes([CANARY] * 4), np.int32)[0])
IMIN, IMAX = -(1 << 31), (1 << 31) - 1
HOP, TAIL = 160, 240


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def items_for(rng, B, max_iv, T):
    """Seeded items (B, max_iv, 2): unsorted, overlapping; most short and inside a window of the row (so that cuts outside it stay
    empty), some long, some empty or reversed, some outside the row on either side, some across its end."""
    iv = np.zeros((B, max_iv, 2), np.int32)
    for b in range(B):
        w = max(int(rng.integers(T // 4, T // 2 + 1)), 1)
        a = int(rng.integers(0, max(T - w, 0) + 1))
        for j in range(max_iv):
            kind = int(rng.integers(0, 20))
            s = int(rng.integers(a, a + w))
            if kind < 12:
                n = int(rng.integers(1, max(T // 16, 2) + 1))
            elif kind < 15:
                n = int(rng.integers(max(T // 16, 2), max(T // 2, 3) + 1))
            elif kind < 17:
                n = int(rng.integers(-3, 1))
            elif kind < 19:
                s, n = (int(rng.integers(-50, -20)), int(rng.integers(1, 20))) if kind == 17 else (T + int(rng.integers(0, 9)), int(rng.integers(1, 20)))
            else:
                s, n = T - 1, int(rng.integers(2, 30))
            iv[b, j] = s, s + n
    return iv


def _run(rt, lab, T, lens, cfg, iv, counts, mode, max_cuts=None, max_pairs=8, with_item_cuts=True, poison_tail=True):
    """labels -> uvad_cuts_table -> (table entries past the cuts taking part poisoned) -> uvad_cuts_join, every output pre-filled with
    the canary, both workspaces full of garbage.  -> dict of host copies with two spare entries (rows) after each output."""
    from uvad_amd import _lib
    lib, ctx = rt.lib, rt.ctx
    q = _lib.CutsCfg(*cfg)
    B, ld = lab.shape
    max_iv = iv.shape[1]
    mc = B * int(lib.uvad_cuts_max_per_row(C.byref(q), T)) if max_cuts is None else max_cuts
    d_lab = torch.from_numpy(np.ascontiguousarray(lab)).to(DEV)
    d_tab = torch.full(((mc + 2) * 32,), CANARY, dtype=torch.uint8, device=DEV)
    d_first = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    d_total = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = max(int(lib.uvad_cuts_ws_bytes(ctx, B, T)), 16)
    ws = torch.full((need,), 0xA7, dtype=torch.uint8, device=DEV)
    d_lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    S = T * cfg[3] + cfg[5]
    code = lib.uvad_cuts_table(ctx, d_lab.data_ptr(), ld, B, T, d_lens.data_ptr() if d_lens is not None else None, None, S, C.byref(q),
                               d_tab.data_ptr(), mc, d_first.data_ptr(), d_total.data_ptr(), ws.data_ptr(), need, None)
    assert code == 0, lib.uvad_last_error(ctx)
    if poison_tail:
        m = min(int(d_total.cpu()[0]), mc)
        bad = np.zeros(mc + 2 - m, cr.CUT_DTYPE)
        bad["n_frames"] = 1 << 30                     # row 0, [0, 2^30): overlaps every item of row 0 were it read
        d_tab[m * 32:] = torch.from_numpy(bad.view(np.uint8).copy()).to(DEV)
    d_iv = torch.from_numpy(np.ascontiguousarray(iv, np.int32)).to(DEV)
    d_cnt = torch.tensor(np.asarray(counts, np.int32), dtype=torch.int32, device=DEV)
    d_pf = torch.full(((mc + 3) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_pairs = torch.full(((max_pairs + 2) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_ic = torch.full((max(B * max_iv * 2, 1) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_aud = torch.full(((B + 2) * 8 * 8,), CANARY, dtype=torch.uint8, device=DEV)
    need = int(lib.uvad_cuts_join_ws_bytes(ctx, B, max_iv, mc))
    assert need >= 16
    jws = torch.full((need,), 0xA7, dtype=torch.uint8, device=DEV)
    code = lib.uvad_cuts_join(ctx, d_tab.data_ptr() if mc else None, d_first.data_ptr(), d_total.data_ptr(), mc, B,
                              d_iv.data_ptr() if max_iv else None, d_cnt.data_ptr(), max_iv, mode, d_pf.data_ptr(),
                              d_pairs.data_ptr() if max_pairs else None, max_pairs, d_ic.data_ptr() if with_item_cuts else None,
                              d_aud.data_ptr(), jws.data_ptr(), need, None)
    assert code == 0, lib.uvad_last_error(ctx)
    torch.cuda.synchronize()
    return {"pair_first": d_pf.cpu().numpy().view(np.int32), "pairs": d_pairs.cpu().numpy().view(np.int32),
            "item_cuts": d_ic.cpu().numpy().view(np.int32)[:B * max_iv * 2].reshape(B, max_iv, 2), "audit": d_aud.cpu().numpy().view(np.uint64).reshape(B + 2, 8),
            "total": int(d_total.cpu()[0]), "row_first": d_first.cpu().numpy(), "max_cuts": mc, "dev": (d_tab, d_first, d_total)}


TABLES = {}


def _table_ref(lab, T, lens, cfg):
    key = (lab.tobytes(), lab.shape, T, None if lens is None else tuple(lens), cfg)
    if key not in TABLES:
        TABLES[key] = cr.table(lab[:, :T], lens, None, T * cfg[3] + cfg[5], cfg)
    return TABLES[key]


def _check(rt, lab, T, lens, cfg, iv, counts, mode, max_cuts=None, max_pairs=None, with_item_cuts=True, spare=3):
    """One table + join on the device against the restatement, everything that must not be read poisoned: byte for byte, canaries
    included, and the audit's two sides against each other.  -> the restatement's answer."""
    want_tab, first = _table_ref(lab, T, lens, cfg)
    B, max_iv = iv.shape[0], iv.shape[1]
    ref = jr.join(want_tab, first, iv, counts, mode, max_cuts=max_cuts, item_cuts=np.full((B, max_iv, 2), CANARY32, np.int32))
    m, total = ref["m"], len(ref["pairs"])
    mp = total + spare if max_pairs is None else max_pairs
    stored = min(total, mp)
    poisoned = np.array(iv, np.int32)
    for b in range(B):
        nb = min(max(int(counts[b]), 0), max_iv)
        poisoned[b, nb:] = IMIN, IMAX
        if min(int(first[b]), m) == min(int(first[b + 1]), m):
            poisoned[b, :] = IMIN, IMAX
    got = _run(rt, lab, T, lens, cfg, poisoned, counts, mode, max_cuts=max_cuts, max_pairs=mp, with_item_cuts=with_item_cuts)
    assert got["total"] == len(want_tab) and np.array_equal(got["row_first"], first)
    assert np.array_equal(got["pair_first"][:m + 1], ref["pair_first"]), (got["pair_first"][:m + 1], ref["pair_first"])
    assert (got["pair_first"][m + 1:] == CANARY32).all()                               # entries past m are not written
    assert np.array_equal(got["pairs"][:stored], ref["pairs"][:stored]) and (got["pairs"][stored:] == CANARY32).all()
    want_items = ref["item_cuts"] if with_item_cuts else np.full((B, max_iv, 2), CANARY32, np.int32)
    assert got["item_cuts"].tobytes() == want_items.tobytes()                          # slots past the counts keep the canary
    assert np.array_equal(got["audit"][:B + 1], ref["audit"]), (got["audit"][:B + 1], ref["audit"])
    assert set(got["audit"][B + 1:].tobytes()) == {CANARY}
    a = got["audit"][:B + 1].astype(np.int64)                                          # consistency, on the device's outputs themselves
    if with_item_cuts:
        for b in range(B):
            nb = min(max(int(counts[b]), 0), max_iv)
            n = got["item_cuts"][b, :nb, 1]
            assert a[b, jr.PAIRS] == int(n.sum()) and a[b, jr.MATCHED] == int((n > 0).sum())
    assert np.array_equal(a[:, jr.UNMATCHED], a[:, jr.ITEMS] - a[:, jr.MATCHED]) and np.array_equal(a[:, jr.REPEATED], a[:, jr.PAIRS] - a[:, jr.MATCHED])
    assert np.array_equal(a[B], a[:B].sum(axis=0)) and a[B, jr.PAIRS] == got["pair_first"][m] == total
    return ref


def _proves_something(ref, mode):
    a = ref["audit"][-1]
    return jr.interesting(ref) if mode == jr.OVERLAP else bool(a[jr.PAIRS] > 0 and a[jr.UNMATCHED] > 0 and a[jr.EMPTY] > 0 and a[jr.EXCEEDING] == 0)


def _mask_padding(rows, T, ld, lens):
    """rows (B, T) -> (B, ld) with every byte at or past each row's length 0xFF (a row of length 0 is 0xFF throughout)."""
    lab = np.full((rows.shape[0], ld), 0xFF, np.uint8)
    for b in range(rows.shape[0]):
        n = T if lens is None else min(max(lens[b], 0), T)
        lab[b, :n] = rows[b, :n]
    return lab


def _sweep_rows(T, seed):
    rng = np.random.default_rng(seed)
    edges = np.zeros(T, np.uint8)
    edges[:max(T // 5, 1)] = 1
    edges[T - max(T // 7, 1):] = 1
    rand = (np.cumsum(rng.random(T) < 0.15) % 2).astype(np.uint8) * np.uint8(3)     # any non-zero byte counts as 1
    blocks = (np.arange(T) % 21 < 6).astype(np.uint8)                                # runs of 6 frames 15 apart: many cuts, with pad 7 one frame apart
    return np.stack([np.zeros(T, np.uint8), np.ones(T, np.uint8), blocks, edges, rand])


def sweep_length_sets(T):
    return (None, [T - 1] * 5, [0, T - 1, T, T // 2, 0], [T + 9, -4, T, 1 << 30, T - 1], [1] * 5)


SWEEP_T = [1, 64, 65, 257, 3001]
SWEEP_ITEMS = [0, 1, 63, 64, 65, 200]
SWEEP_CFGS = [(P, W, m, HOP, 0, TAIL) for P in (0, 7) for W, m in ((0, 0), (50, 5))]
# the seed of each (T, items per row) shape's items, chosen on the CPU (the lowest from 1 up) so that the restatement's answer meets
# _proves_something in both modes, for every configuration and every length set that is not exempt
SWEEP_SEEDS = {(64, 63): 3, (64, 64): 1, (64, 65): 3, (64, 200): 1, (65, 63): 3, (65, 64): 1, (65, 65): 3, (65, 200): 1, (257, 63): 1, (257, 64): 1,
               (257, 65): 1, (257, 200): 1, (3001, 63): 1, (3001, 64): 1, (3001, 65): 2, (3001, 200): 1}


def sweep_case(T, n_items, seed):
    """-> (rows, items, counts): counts vary around n_items and reach past max_iv and below 0 (clamped)."""
    rows = _sweep_rows(T, 100 + T)
    rng = np.random.default_rng(seed)
    iv = items_for(rng, 5, n_items, T)
    counts = [n_items, n_items + 5, max(n_items - 1, 0), n_items, -3 if n_items > 64 else n_items]
    return rows, iv, counts


def sweep_exempt(T, n_items, lens):
    return T == 1 or n_items < 2 or (lens is not None and max(lens) <= 1)


@pytest.mark.parametrize("T", SWEEP_T)
@pytest.mark.parametrize("mode", [jr.OVERLAP, jr.INSIDE])
def test_sweep_equals_the_restatement(rt, mode, T):
    cases = proving = 0
    for n_items in SWEEP_ITEMS:
        rows, iv, counts = sweep_case(T, n_items, SWEEP_SEEDS.get((T, n_items), 0))
        for cfg in SWEEP_CFGS:
            for lens in sweep_length_sets(T):
                ref = _check(rt, _mask_padding(rows, T, T + 3, lens), T, lens, cfg, iv, counts, mode)
                if not sweep_exempt(T, n_items, lens):
                    assert _proves_something(ref, mode), (T, n_items, cfg, lens, ref["audit"][-1])
                    proving += 1
                cases += 1
    assert cases == 6 * 4 * 5 and proving == (0 if T == 1 else 4 * 4 * 4)


def _hand_labels(T, cuts):
    row = np.zeros(T, np.uint8)
    for f, k in cuts:
        row[f:f + k] = 1
    return row


@pytest.mark.parametrize("mode", [jr.OVERLAP, jr.INSIDE])
def test_borders_on_ballot_word_boundaries(rt, mode):
    """The hand-made answers of tests/test_join_ref.py with the cut borders on frames 64 / 128 / 192 (row 0), 63 / 127 / 191 (row 1) and
    65 / 129 / 193 (row 2): pad 0 and pieces of 64 frames make the run [a - 64, a + 128) three adjacent cuts, then a gap and one more cut."""
    T = 320
    rows, ivs = [], []
    for d in (0, -1, 1):
        a = 128 + d                                   # cuts [a - 64, a) [a, a + 64) [a + 64, a + 128) and [270, 280)
        rows.append(_hand_labels(T, [(a - 64, 192), (270, 10)]))
        ivs.append([(a - 64, a), (a, a + 64), (a - 1, a), (a - 1, a + 1), (a, a + 1), (a + 63, a + 65), (a + 64, a + 64), (a + 64, a + 63),
                    (a - 10, a + 70), (a - 64, a + 128), (a + 128, 270), (a + 127, 270), (a + 128, 271), (270, 280), (269, 280), (270, 281),
                    (280, 290), (279, 290), (-5, a - 64), (-5, a - 63), (275, 1000), (IMIN, IMAX), (a + 10, a + 20)])
    iv = np.asarray(ivs, np.int64).astype(np.int32)
    lab = np.stack(rows)
    ref = _check(rt, lab, T, None, (0, 64, 0, HOP, 0, TAIL), iv, [iv.shape[1]] * 3, mode)
    tab, first = _table_ref(lab, T, None, (0, 64, 0, HOP, 0, TAIL))
    assert [(int(c["first_frame"]), int(c["n_frames"])) for c in tab[:4]] == [(64, 64), (128, 64), (192, 64), (270, 10)] and len(tab) == 12
    ic = ref["item_cuts"][0].tolist()
    if mode == jr.OVERLAP:                            # row 0, a = 128: known answers
        assert ic[:10] == [[0, 1], [1, 1], [0, 1], [0, 2], [1, 1], [1, 2], [-1, 0], [-1, 0], [0, 3], [0, 3]]
        assert ic[10:17] == [[-1, 0], [2, 1], [3, 1], [3, 1], [3, 1], [3, 1], [-1, 0]] and ic[17:] == [[3, 1], [-1, 0], [0, 1], [3, 1], [0, 4], [1, 1]]
        assert int(ref["audit"][-1][jr.REPEATED]) > 0 and int(ref["audit"][-1][jr.EXCEEDING]) > 0 and int(ref["audit"][-1][jr.UNMATCHED]) > 0
    else:
        assert ic[:10] == [[0, 1], [1, 1], [0, 1], [-1, 0], [1, 1], [-1, 0], [-1, 0], [-1, 0], [-1, 0], [-1, 0]]
        assert ic[10:17] == [[-1, 0], [-1, 0], [-1, 0], [3, 1], [-1, 0], [-1, 0], [-1, 0]] and ic[17:] == [[-1, 0], [-1, 0], [-1, 0], [-1, 0], [-1, 0], [1, 1]]
        assert int(ref["audit"][-1][jr.EXCEEDING]) == 0 and int(ref["audit"][-1][jr.REPEATED]) == 0


@pytest.mark.parametrize("mode", [jr.OVERLAP, jr.INSIDE])
def test_many_cuts_in_one_row(rt, mode):
    T = 700                                           # alternating labels, pad 0: 350 cuts of one frame, more than 64 and more than 256
    lab = np.stack([((np.arange(T) + 1) % 2).astype(np.uint8), (np.arange(T) % 2).astype(np.uint8)])      # row 0: cut i is frame 2 i
    rng = np.random.default_rng(11)
    iv = items_for(rng, 2, 150, T)
    iv[0, :4] = [[0, T], [1, 2], [0, 1], [300, 301]]  # every cut of row 0; the gap after its first cut; its first cut; cut 150
    ref = _check(rt, lab, T, None, (0, 0, 0, HOP, 0, TAIL), iv, [150, 149], mode)
    assert int(ref["audit"][0][jr.CUTS]) == 350 and int(ref["audit"][1][jr.CUTS]) == 350 and _proves_something(ref, mode)
    assert ref["item_cuts"][0, :4].tolist() == ([[0, 350], [-1, 0], [0, 1], [150, 1]] if mode == jr.OVERLAP else [[-1, 0], [-1, 0], [0, 1], [150, 1]])


@pytest.mark.parametrize("mode", [jr.OVERLAP, jr.INSIDE])
def test_many_rows(rt, mode):
    rng = np.random.default_rng(7)
    B, T = 1030, 9                                    # more than 256 cuts per scan round, over several rounds; row B sums 1030 rows
    rows = (rng.random((B, T)) < 0.45).astype(np.uint8)
    lens = rng.integers(0, T + 1, B).tolist()
    iv = np.zeros((B, 3, 2), np.int32)
    iv[:, :, 0] = rng.integers(-2, T, (B, 3))
    iv[:, :, 1] = iv[:, :, 0] + rng.integers(0, 5, (B, 3))
    counts = rng.integers(0, 4, B).tolist()
    ref = _check(rt, _mask_padding(rows, T, T, lens), T, lens, (0, 3, 0, HOP, 0, TAIL), iv, counts, mode)
    assert ref["m"] > 1030 and _proves_something(ref, mode)


@pytest.mark.parametrize("mode", [jr.OVERLAP, jr.INSIDE])
def test_long_row(rt, mode):
    T = 20011
    rng = np.random.default_rng(8)
    row = (np.cumsum(rng.random(T) < 0.2) % 2).astype(np.uint8)
    iv = items_for(rng, 1, 1000, T)
    ref = _check(rt, row[None, :], T, None, (2, 7, 1, HOP, 0, TAIL), iv, [1000], mode)
    assert ref["m"] > 2000 and _proves_something(ref, mode)


def _trunc_case():
    T = 257
    rows = _sweep_rows(T, 3)
    iv = items_for(np.random.default_rng(5), 5, 40, T)
    return T, rows, iv, [40, 31, 40, 0, 17], (1, 5, 2, HOP, 0, TAIL)


def test_max_pairs_below_the_total(rt):
    T, rows, iv, counts, cfg = _trunc_case()
    full = _check(rt, rows, T, None, cfg, iv, counts, jr.OVERLAP)
    total = len(full["pairs"])
    assert total > 60 and _proves_something(full, jr.OVERLAP)
    for mp in (0, 1, total // 2, total - 1, total):
        ref = _check(rt, rows, T, None, cfg, iv, counts, jr.OVERLAP, max_pairs=mp)    # pair_first and the audit stay true; the canary after the stored pairs is intact
        assert np.array_equal(ref["audit"], full["audit"])


def test_max_cuts_below_the_table_total(rt):
    T, rows, iv, counts, cfg = _trunc_case()
    full = _check(rt, rows, T, None, cfg, iv, counts, jr.OVERLAP)
    n_cuts = full["m"]
    assert n_cuts > 40
    for mc in (0, 1, 17, 60, n_cuts - 1, n_cuts):
        ref = _check(rt, rows, T, None, cfg, iv, counts, jr.OVERLAP, max_cuts=mc)     # the join sees only the stored cuts
        assert ref["m"] == mc and int(ref["audit"][-1][jr.CUTS]) == mc
    assert int(_check(rt, rows, T, None, cfg, iv, counts, jr.INSIDE, max_cuts=17)["audit"][-1][jr.CUTS]) == 17


def test_null_item_cuts_and_no_items(rt):
    T, rows, iv, counts, cfg = _trunc_case()
    for mode in (jr.OVERLAP, jr.INSIDE):
        _check(rt, rows, T, None, cfg, iv, counts, mode, with_item_cuts=False)
        ref = _check(rt, rows, T, None, cfg, iv[:, :0], [0] * 5, mode)                # max_iv = 0: d_iv is NULL
        assert int(ref["audit"][-1][jr.ITEMS]) == 0 and int(ref["audit"][-1][jr.EMPTY]) == ref["m"] > 0
        ref = _check(rt, rows, T, None, cfg, iv, [0] * 5, mode)                       # every slot poisoned, none read
        assert int(ref["audit"][-1][jr.PAIRS]) == 0


def test_what_is_never_read_was_really_poisoned(rt):
    """The poison of _check is not vacuous: without it (the restatement given the poisoned items as real ones) the answer differs."""
    T, rows, iv, counts, cfg = _trunc_case()
    want_tab, first = _table_ref(rows, T, None, cfg)
    assert first[3] < first[4] and counts[3] == 0 and counts[1] < iv.shape[1]        # a row with cuts and no items; a row with spare slots
    assert first[0] == first[1]                                                       # a row without cuts, whose item slots are all poisoned
    ref = _check(rt, rows, T, None, cfg, iv, counts, jr.OVERLAP, max_cuts=17)
    bad = np.array(iv)
    bad[1, counts[1]:] = IMIN, IMAX
    worse = jr.join(want_tab, first, bad, [40] * 5, jr.OVERLAP, max_cuts=17)
    assert int(worse["audit"][-1][jr.PAIRS]) > int(ref["audit"][-1][jr.PAIRS])


def test_same_calls_same_bytes(rt):
    T, rows, iv, counts, cfg = _trunc_case()
    outs = []
    for _ in range(2):
        g = _run(rt, rows, T, None, cfg, iv, counts, jr.OVERLAP, max_pairs=100)
        outs.append((g["pair_first"].tobytes(), g["pairs"].tobytes(), g["item_cuts"].tobytes(), g["audit"].tobytes()))
    assert outs[0] == outs[1]


def test_one_captured_graph_replays_with_new_inputs(rt):
    B, T, S, max_iv = 3, 700, 700 * 160 + 240, 48
    cfg = dict(pad=4, max_len=60, min_len=3, hop=160, lead=0, tail=240)
    rng = np.random.default_rng(31)
    batches = []
    for k in range(3):
        lab = (np.cumsum(rng.random((B, T)) < (0.02, 0.1, 0.3)[k], axis=1) % 2).astype(np.uint8)
        lens = [[T, 64, 0], [1, T - 1, 333], [650, 0, T]][k]
        nsamp = [[S, 64 * 160, 0], [400, S - 5, 333 * 160 + 240], [S, 0, 50000]][k]
        pcm = rng.integers(-30000, 30000, (B, S)).astype(np.int16)
        batches.append((lab, lens, nsamp, pcm, items_for(rng, B, max_iv, T), [[48, 20, 48], [0, 48, 31], [48, 48, 5]][k]))
    s_lab = torch.zeros((B, T), dtype=torch.uint8, device=DEV)
    s_len = torch.zeros(B, dtype=torch.int32, device=DEV)
    s_ns = torch.zeros(B, dtype=torch.int64, device=DEV)
    s_pcm = torch.zeros((B, S), dtype=torch.int16, device=DEV)
    s_iv = torch.zeros((B, max_iv, 2), dtype=torch.int32, device=DEV)
    s_cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    ct = rt.cuts_open(**cfg)
    rt.speech_cuts(s_lab, s_pcm, lengths=s_len, nsamp=s_ns, cuts=ct)                    # sizes the buffers; no cut
    rt.cuts_join(ct, s_iv, s_cnt, mode="overlap", max_pairs=4000)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                      # one stream; a synchronisation or allocation in the calls would fail here
        table, _, _ = rt.cuts_table(s_lab, lengths=s_len, nsamp=s_ns, S=S, cuts=ct)
        out = rt.cuts_join(ct, s_iv, s_cnt, mode="overlap", max_pairs=4000)
        batch, lens_out = rt.cuts_gather(s_pcm, ct, "samples")
    ld_out = batch.shape[1]
    totals = []
    for lab, lens, nsamp, pcm, iv, counts in batches:
        s_lab.copy_(torch.from_numpy(lab).to(DEV))
        s_len.copy_(torch.tensor(lens, dtype=torch.int32, device=DEV))
        s_ns.copy_(torch.tensor(nsamp, dtype=torch.int64, device=DEV))
        s_pcm.copy_(torch.from_numpy(pcm).to(DEV))
        s_iv.copy_(torch.from_numpy(iv).to(DEV))
        s_cnt.copy_(torch.tensor(counts, dtype=torch.int32, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        want, first = cr.table(lab, lens, nsamp, S, tuple(cfg.values()))
        ref = jr.join(want, first, iv, counts, jr.OVERLAP)
        n, total = len(want), len(ref["pairs"])
        totals.append(total)
        assert rt.cuts_read(ct).tobytes() == want.tobytes()
        assert np.array_equal(out["pair_first"][:n + 1].cpu().numpy(), ref["pair_first"]) and total <= 4000
        assert np.array_equal(out["pairs"][:total].cpu().numpy(), ref["pairs"])
        assert np.array_equal(out["audit"].cpu().numpy().astype(np.uint64), ref["audit"])
        got_ic = out["item_cuts"].cpu().numpy()
        for b in range(B):
            assert np.array_equal(got_ic[b, :counts[b]], ref["item_cuts"][b, :counts[b]])
        ref_out, ref_len = cr.gather(pcm, want, "samples", ld_out, np.zeros((n, ld_out), np.int16), np.zeros(n, np.int32))
        assert np.array_equal(batch[:n].cpu().numpy(), ref_out) and np.array_equal(lens_out[:n].cpu().numpy(), ref_len)
        assert _proves_something(ref, jr.OVERLAP)
    assert min(totals) > 0 and len(set(totals)) == 3


def test_host_layer(rt):
    T, rows, iv, counts, cfg = _trunc_case()
    counts = [min(c, 40) for c in counts]
    want_tab, first = _table_ref(rows, T, None, cfg)
    ct = rt.cuts_open(**dict(zip(("pad", "max_len", "min_len", "hop", "lead", "tail"), cfg)))
    with pytest.raises(RuntimeError):
        rt.cuts_join(ct, iv, counts)                                                   # no table yet
    rt.cuts_table(torch.from_numpy(rows).to(DEV), cuts=ct)
    with pytest.raises(ValueError):
        rt.cuts_join(ct, iv, counts, mode="within")
    with pytest.raises(ValueError):
        rt.cuts_join(ct, iv[:4], counts[:4])
    for mode, code in (("overlap", jr.OVERLAP), ("inside", jr.INSIDE)):
        ref = jr.join(want_tab, first, iv, counts, code)
        out = rt.cuts_join(ct, iv, counts, mode=mode)                                  # numpy in, device tensors out
        assert all(torch.is_tensor(t) and t.device == DEV for t in out.values()) and set(out) == {"pair_first", "pairs", "item_cuts", "audit"}
        assert out["pairs"].numel() == min(ct["max_cuts"] * 40, ct["max_cuts"] + 5 * 40) >= len(ref["pairs"])
        read = rt.cuts_join_read(ct)
        assert read["pairs_per_cut"] == ref["per_cut"] and read["total_pairs"] == read["stored_pairs"] == len(ref["pairs"])
        assert np.array_equal(read["audit_words"].astype(np.uint64), ref["audit"])
        names = dict(rt.JOIN_AUDIT_NAMES)
        assert read["audit"]["pooled"] == {n: int(ref["audit"][-1][k]) for n, k in names.items()}
        assert [r["Total Supervisions"] for r in read["audit"]["rows"]] == counts and len(read["audit"]["rows"]) == 5
        for b in range(5):
            assert np.array_equal(read["item_cuts"][b, :counts[b]], ref["item_cuts"][b, :counts[b]])
    small = rt.cuts_join(ct, torch.from_numpy(iv).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), max_pairs=7, rows=60)
    ref = jr.join(want_tab, first, iv, counts, jr.OVERLAP, max_cuts=60, max_pairs=7)
    read = rt.cuts_join_read(ct)
    assert small["pairs"].numel() == 7 and read["stored_pairs"] == 7 and read["total_pairs"] == len(ref["pairs"]) > 7
    assert len(read["pairs_per_cut"]) == 60 and sum(read["pairs_per_cut"], []) == ref["stored"].tolist()
    assert np.array_equal(read["audit_words"].astype(np.uint64), ref["audit"])


def _predict_with_supervisions(tmp_path, shift, geometry):
    """predict_vad(cuts=..., supervisions=..., alignments=...) on two synthetic 12 s recordings: transcripts, indices and audit against
    the same join made on the host from the cut table the results carry; without the new options nothing changes."""
    from config.config import load_config
    from src.scripts import predict_vad
    from uvad_amd.postprocess import cut_transcripts, join_report, supervision_frames
    from uvad_amd.runtime import VadRuntime
    cfg = load_config()
    if cfg.feature_extractor == "fbank":
        cfg.model_dict.encoding_dim = 64
    cfg.input.kind = "synthetic"
    cfg.input.num_utterances = 2
    cfg.input.seconds = 12.0
    cfg.input.seed = 77
    cfg.max_duration = 60
    assert cfg.supervisions is None and cfg.alignments is None
    cfg.cuts = {"buffer": 0.1, "split": True, "window": 2.0, "min": 0.1}
    plain = predict_vad(**cfg)                                                         # what the parent commit returns
    assert [set(r) for r in plain] == [{"recording_id", "num_frames", "labels", "probs", "intervals", "cuts"}] * 2
    assert all(isinstance(c, tuple) and len(c) == 4 for r in plain for c in r["cuts"])
    with pytest.raises(ValueError):
        predict_vad(**{**cfg, "cuts": None, "supervisions": {}})
    ids = [r["recording_id"] for r in plain]
    sup0 = [(0.0, 1.5, "zero"), (1.0, 4.25, "one"), (4.25, 4.25, "empty"), (5.0, 11.0, None), (11.5, 12.0, "last"), (30.0, 31.0, "outside")]
    path = tmp_path / "sup1.txt"
    path.write_text("".join(f"{0.7 * k:.2f}\t{0.7 * k + 0.5:.2f}\tw{k} x\n" for k in range(17)))
    words0 = [(0.25 * k, 0.25 * k + 0.2, f"a{k}") for k in range(48)]
    cfg.supervisions = {ids[0]: sup0, ids[1]: str(path)}
    cfg.alignments = {ids[0]: words0}                                                  # recording 1 has no alignment: no words
    got = predict_vad(**cfg)
    sup1 = [(round(0.7 * k, 2), round(0.7 * k + 0.5, 2), f"w{k} x") for k in range(17)]
    pooled, n_cuts = np.zeros(8, np.int64), 0
    for k, (g, p) in enumerate(zip(got, plain)):
        assert set(g) == set(p) | {"audit", "audit_words"}
        for key in p:
            if key != "cuts":
                assert np.array_equal(g[key], p[key]) if isinstance(p[key], np.ndarray) else g[key] == p[key], key
        assert [(c["start"], c["end"], c["first_sample"], c["n_samples"]) for c in g["cuts"]] == p["cuts"]
        nf = g["num_frames"]
        tab = np.array([(0, i, round(c[0] / shift), round(c[1] / shift) - round(c[0] / shift), c[2], c[3]) for i, c in enumerate(p["cuts"])], dtype=cr.CUT_DTYPE).reshape(-1)
        first = np.asarray([0, len(tab)], np.int32)
        for source, name, mode, key in (((sup0, sup1)[k], "supervisions", jr.OVERLAP, "audit"), ((words0, [])[k], "words", jr.INSIDE, "audit_words")):
            frames = supervision_frames([(s, e) for s, e, _ in source], 12.0, frame_shift=shift, geometry=geometry, num_frames=nf).reshape(1, -1, 2)
            ref = jr.join(tab, first, frames, [len(source)], mode)
            assert [c[name] for c in g["cuts"]] == ref["per_cut"]
            if (name == "words") == (k == 0):                                          # recording 0 has an alignment: its words are the text
                assert [c["text"] for c in g["cuts"]] == cut_transcripts(ref["per_cut"], [t for _, _, t in source])
            names = dict(VadRuntime.JOIN_AUDIT_NAMES)
            assert g[key] == {n: int(ref["audit"][0][w]) for n, w in names.items()}, (k, name)
            if name == "supervisions":
                pooled += ref["audit"][0].astype(np.int64)
        n_cuts += len(g["cuts"])
    assert n_cuts >= 2 and pooled[jr.PAIRS] > 0 and pooled[jr.UNMATCHED] > 0
    total = {n: sum(g["audit"][n] for g in got) for n in got[0]["audit"]}
    text = join_report(total, "synthetic", 0.1, "test")
    assert f"Total Supervisions: {len(sup0) + len(sup1)}\n" in text and f"Supervisions in new cuts: {int(pooled[jr.PAIRS])}\n" in text
    print(text)


def test_predict_vad_with_supervisions(tmp_path):
    _predict_with_supervisions(tmp_path, 0.01, "fbank")


def test_predict_vad_with_supervisions_sincnet(tmp_path, monkeypatch):
    monkeypatch.setenv("UVAD_FEATURE_EXTRACTOR", "sincnet")
    _predict_with_supervisions(tmp_path, 270 / 16000.0, "sincnet")
