"""Channel fusion on the device (uvad_fuse, uvad_fuse_pick; include/uvad.h) against the numpy restatement tests/fuse_ref.py, byte for byte:
a sweep of small shapes over the three modes, weights, length sets, row strides and a misaligned base; the group layouts; NaN, +-inf,
values exactly at threshold and decide; a long row, many groups; the accumulating counters; determinism; every optional output NULL in
turn; one captured graph of fuse + table + pick + gather replayed with new inputs; the pick's borders; composition with binarize and
scoring; the host layer.

EVERY comparison below (_run + _check) runs with what must never be read poisoned with NaN -- input columns at or past a row's length,
rows no group names, whole rows of length 0, the slack between rows: a NaN read there would surface as a NaN fused value, a label of 1
and a best position -- and with every output pre-filled with a canary that must survive wherever the header says "not written": columns
at or past the group's length, a spare row and a spare column after every output.  The workspace is full of garbage."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuts_ref as cr
import fuse_ref as fr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY = 0x5A
VALUES = np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)      # few values: ties are frequent, 0.5 sits on threshold and decide
MODES = (fr.MAX, fr.MEAN, fr.VOTE)


@pytest.fixture(scope="module")
def rt():
    import uvad_amd
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                      # no feature tables, weights or model: a post-processing context
    yield r
    r.close()


def configure(rt, groups, mode, thr=0.5, dec=0.5, weights=None):
    from uvad_amd import _lib
    first = np.zeros(len(groups) + 1, np.int32)
    first[1:] = np.cumsum([len(g) for g in groups])
    members = np.ascontiguousarray(np.concatenate([np.asarray(g, np.int32) for g in groups]))
    w = None if weights is None else np.ascontiguousarray(np.concatenate([np.asarray(v, np.float32) for v in weights]))
    q = _lib.FuseCfg(mode, thr, dec)
    code = rt.lib.uvad_fuse_configure(rt.ctx, C.byref(q), first.ctypes.data, members.ctypes.data, w.ctypes.data if w is not None else None,
                                      len(groups))
    assert code == 0, rt.lib.uvad_last_error(rt.ctx)
    rt._fuse_current = None                  # the host layer's memo of what the context holds
    return int(first[-1])


def values(rng, B, T, nan=0.01):
    x = VALUES[rng.integers(0, len(VALUES), (B, T))]
    x[rng.random((B, T)) < nan] = np.nan
    return x


def _run(rt, x, groups, T, lens=None, ld_in=None, off=0, flags=None, labels=True, best=True, stats=True, stats_init=None, N=None):
    """One uvad_fuse on the configuration the context holds.  -> dict of host copies, each with a spare row and a spare column."""
    lib, ctx = rt.lib, rt.ctx
    B, G = x.shape[0], len(groups)
    N = sum(len(g) for g in groups) if N is None else N
    ld_in = T if ld_in is None else ld_in
    named = {r for g in groups for r in g}
    host = np.full(off + B * ld_in + 8, np.nan, np.float32)
    for r in range(B):
        n = T if lens is None else min(max(int(lens[r]), 0), T)
        if r in named and n > 0:
            host[off + r * ld_in: off + r * ld_in + n] = x[r, :n]
    d_in = torch.from_numpy(host).to(DEV)
    d_lens = None if lens is None else torch.tensor(np.asarray(lens, np.int32), dtype=torch.int32, device=DEV)
    d_fl = None if flags is None else torch.tensor(np.asarray(flags, np.uint8), dtype=torch.uint8, device=DEV)
    ld = T + 1
    d_f = torch.full(((G + 1) * ld * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_gl = torch.full(((G + 1) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_fo = torch.full((G + 1,), CANARY, dtype=torch.uint8, device=DEV)
    d_lab = torch.full(((G + 1) * ld,), CANARY, dtype=torch.uint8, device=DEV)
    d_best = torch.full(((G + 1) * ld,), CANARY, dtype=torch.uint8, device=DEV)
    init = np.zeros((N + 1, 4), np.uint64) if stats_init is None else stats_init
    d_st = torch.from_numpy(init.view(np.int64).copy()).to(DEV)
    need = int(lib.uvad_fuse_ws_bytes(ctx, B, T))
    assert need >= 16
    ws = torch.full((need,), 0xA7, dtype=torch.uint8, device=DEV)
    code = lib.uvad_fuse(ctx, d_in.data_ptr() + 4 * off, ld_in, B, T, d_lens.data_ptr() if d_lens is not None else None,
                         d_fl.data_ptr() if d_fl is not None else None, d_f.data_ptr(), ld, d_gl.data_ptr(),
                         d_fo.data_ptr() if d_fl is not None else None, d_lab.data_ptr() if labels else None, ld,
                         d_best.data_ptr() if best else None, ld, d_st.data_ptr() if stats else None, ws.data_ptr(), need, None)
    assert code == 0, lib.uvad_last_error(ctx)
    torch.cuda.synchronize()
    return {"fused": d_f.cpu().numpy().reshape(G + 1, ld * 4), "glens": d_gl.cpu().numpy().view(np.int32), "flags": d_fo.cpu().numpy(),
            "labels": d_lab.cpu().numpy().reshape(G + 1, ld), "best": d_best.cpu().numpy().reshape(G + 1, ld),
            "stats": d_st.cpu().numpy().view(np.uint64), "dev": (d_in, d_f, d_lab, d_best, d_gl)}


def _check(got, ref, T, labels=True, best=True, stats=True, flags=False, stats_init=None, what=""):
    G = len(ref["glens"])
    assert got["glens"][:G].tolist() == ref["glens"].tolist(), what
    assert got["glens"][G:].tobytes() == bytes([CANARY] * 4), what
    for g in range(G):
        L = int(ref["glens"][g])
        assert got["fused"][g, :4 * L].tobytes() == ref["fused"][g, :L].tobytes(), (what, g)
        assert (got["fused"][g, 4 * L:] == CANARY).all(), (what, g)          # past the group's length, and the spare column
        for name, on in (("labels", labels), ("best", best)):
            if on:
                assert got[name][g, :L].tobytes() == ref[name][g, :L].tobytes(), (what, name, g)
            assert (got[name][g, L if on else 0:] == CANARY).all(), (what, name, g)
    for name in ("fused", "labels", "best"):
        assert (got[name][G] == CANARY).all(), (what, name)                   # the spare row
    N = ref["stats"].shape[0]
    base = np.zeros((N + 1, 4), np.uint64) if stats_init is None else stats_init
    want = base.copy()
    if stats:
        want[:N] += ref["stats"]
    assert got["stats"].tobytes() == want.tobytes(), what
    if flags:
        assert got["flags"][:G].tolist() == ref["flags"].tolist() and got["flags"][G] == CANARY, what
    else:
        assert (got["flags"] == CANARY).all(), what
    if stats and stats_init is None:
        # the slot side against the group side, on the device's outputs alone: every frame below a group's length has exactly one best member
        assert int(got["stats"][:N, 3].sum()) == int(got["glens"][:G].sum()), what


def length_sets(rng, groups, B, T):
    """dense; all equal and short; ragged within a group; one member of length 0; a whole group of length 0."""
    short = np.full(B, max(T // 3, 1), np.int32)
    ragged = rng.integers(1, T + 1, B).astype(np.int32)
    one0 = rng.integers(1, T + 1, B).astype(np.int32)
    one0[groups[0][-1]] = 0
    grp0 = rng.integers(1, T + 1, B).astype(np.int32)
    grp0[groups[len(groups) // 2]] = 0
    grp0[groups[0][0]] = T
    return {"dense": None, "short": short, "ragged": ragged, "one0": one0, "grp0": grp0}


def random_weights(rng, groups):
    out = []
    for g in groups:
        w = rng.choice(np.array([0.0, 0.0, 0.5, 1.0, 2.0, 0.3], np.float32), len(g))
        if not w.sum() > 0:
            w[int(rng.integers(0, len(g)))] = 1.0
        out.append(w.tolist())
    return out


@pytest.mark.parametrize("M", [1, 2, 3, 8, 64, 255])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 257, 3001])
def test_small_shape_sweep(rt, T, M):
    G = 3 if M <= 8 else 2
    B = G * M + 1                                                # the last row belongs to no group
    groups = [list(range(g * M, (g + 1) * M)) for g in range(G)]
    rng = np.random.default_rng(1000 * T + M)
    x = values(rng, B, T)
    sets = length_sets(rng, groups, B, T)
    for mode in MODES:
        for weights in (None, random_weights(rng, groups)):
            configure(rt, groups, mode, 0.5, 0.5, weights)
            for name, lens in sets.items():
                ref = fr.fuse_ref(x, groups, mode, 0.5, 0.5, lens, weights)
                for ld_in, off in ((T, 0), (T + 3, 0), (T, 1), (T + 3, 1)):
                    got = _run(rt, x, groups, T, lens, ld_in, off)
                    _check(got, ref, T, what=(mode, weights is not None, name, ld_in, off))


def test_the_sweep_meets_the_rules_it_is_there_for():
    """On the restatement alone: the sweep's data hold ties, NaN, a zero total weight at a frame, values on threshold and on decide."""
    T, M, G = 257, 3, 3
    groups = [list(range(g * M, (g + 1) * M)) for g in range(G)]
    rng = np.random.default_rng(1000 * T + M)
    x = values(rng, G * M + 1, T)
    sets = length_sets(rng, groups, G * M + 1, T)
    ref = fr.fuse_ref(x, groups, fr.MAX, 0.5, 0.5, sets["ragged"])
    assert np.isnan(ref["fused"]).any() and (ref["fused"] == 0.5).any() and len(set(ref["best"].ravel().tolist())) == M
    x0 = np.nan_to_num(x[:, :T], nan=2.0)
    assert ((x0[0] == x0[1]) & (x0[0] >= x0[2])).any()                       # a tie for best between positions 0 and 1
    w = [[0.0, 1.0, 1.0]] * G
    lens = np.full(G * M + 1, 5, np.int32)
    lens[0] = T
    r2 = fr.fuse_ref(x, groups, fr.MEAN, 0.5, 0.5, lens, w)
    assert (r2["fused"][0, 5:] == 0.0).all() and r2["labels"][0, 5:].sum() == 0   # W == 0 past frame 5 of group 0


def test_group_layouts(rt):
    T, F, Cn = 130, 4, 3
    rng = np.random.default_rng(7)
    x = values(rng, F * Cn + 2, T)
    lens = rng.integers(1, T + 1, F * Cn + 2).astype(np.int32)
    layouts = {"file-major": [[f * Cn + c for c in range(Cn)] for f in range(F)],
               "channel-major": [[c * F + f for c in range(Cn)] for f in range(F)],
               "a row in two groups": [[0, 1, 2], [2, 3], [5, 1, 9, 2]],
               "rows in no group, unordered": [[11, 4], [8], [6, 13, 0]]}
    for name, groups in layouts.items():
        for mode in MODES:
            configure(rt, groups, mode, 0.5, 0.5)
            flags = rng.integers(0, 4, x.shape[0]).astype(np.uint8)
            ref = fr.fuse_ref(x, groups, mode, 0.5, 0.5, lens, flags=flags)
            _check(_run(rt, x, groups, T, lens, T + 1, 0, flags=flags), ref, T, flags=True, what=(name, mode))


def test_logits_with_infinities_and_other_thresholds(rt):
    T, groups = 300, [[0, 1, 2, 3], [4, 5]]
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((6, T)) * 4).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.inf
    x[rng.random(x.shape) < 0.05] = -np.inf
    x[rng.random(x.shape) < 0.01] = np.nan
    lens = np.array([T, 290, 17, T, 64, 65], np.int32)
    weights = [[1.0, 0.0, 2.5, 0.25], [0.5, 0.5]]
    for mode, thr, dec in ((fr.MEAN, 0.0, 0.0), (fr.MEAN, -1.5, 0.75), (fr.MAX, 0.0, 1.0), (fr.VOTE, 0.0, 0.5), (fr.VOTE, 0.0, 1e-6),
                           (fr.VOTE, 1.0, 1.0)):
        for w in (None, weights):
            configure(rt, groups, mode, thr, dec, w)
            ref = fr.fuse_ref(x, groups, mode, thr, dec, lens, w)
            if mode == fr.MEAN:
                assert np.isnan(ref["fused"]).any() and np.isinf(ref["fused"]).any()    # inf - inf and inf x 0 occur, and plain inf
            _check(_run(rt, x, groups, T, lens), ref, T, what=(mode, thr, dec, w is not None))


def test_vote_majority_and_any_member(rt):
    x = np.array([[1, 0, 1, 0], [0, 0, 1, 1], [0, 0, 1, 1]], np.float32)
    configure(rt, [[0, 1], [0, 1, 2]], fr.VOTE, 0.5, 0.5)
    got = _run(rt, x, [[0, 1], [0, 1, 2]], 4)
    assert got["labels"][0, :4].tolist() == [1, 0, 1, 1] and got["labels"][1, :4].tolist() == [0, 0, 1, 1]
    assert got["fused"][0, :16].view(np.float32).tolist() == [0.5, 0.0, 1.0, 0.5]
    configure(rt, [[0, 1, 2]], fr.VOTE, 0.5, 1e-6)
    assert _run(rt, x, [[0, 1, 2]], 4)["labels"][0, :4].tolist() == [1, 0, 1, 1]


def test_a_long_row_and_many_groups(rt):
    rng = np.random.default_rng(5)
    T = 20011                                                    # 20 tiles of 1024 frames; the last holds 555
    x = values(rng, 8, T)
    lens = np.array([T, T - 1, 1024, 1025, 4097, 0, 19999, 3], np.int32)
    for mode in MODES:
        configure(rt, [list(range(8))], mode, 0.5, 0.5)
        _check(_run(rt, x, [list(range(8))], T, lens, T + 1, 1), fr.fuse_ref(x, [list(range(8))], mode, 0.5, 0.5, lens), T, what=mode)
    G, T = 1030, 65
    groups = [[2 * g, 2 * g + 1] for g in range(G)]
    x = values(rng, 2 * G, T)
    lens = rng.integers(0, T + 1, 2 * G).astype(np.int32)
    configure(rt, groups, fr.MEAN, 0.5, 0.5)
    _check(_run(rt, x, groups, T, lens), fr.fuse_ref(x, groups, fr.MEAN, 0.5, 0.5, lens), T, what="1030 groups")


def test_stats_accumulate_and_both_sides_agree(rt):
    T, groups = 1500, [[0, 1, 2], [3, 4], [5]]
    rng = np.random.default_rng(3)
    configure(rt, groups, fr.MAX, 0.5, 0.5)
    total = np.zeros((7, 4), np.uint64)
    total[6] = 77                                                # the spare slot: never touched
    for call in range(2):
        x = values(rng, 6, T)
        lens = rng.integers(1, T + 1, 6).astype(np.int32)
        ref = fr.fuse_ref(x, groups, fr.MAX, 0.5, 0.5, lens)
        got = _run(rt, x, groups, T, lens, stats_init=total.copy())
        _check(got, ref, T, stats_init=total, what=call)
        total = got["stats"].reshape(7, 4).copy()
        # this call alone: valid equals n_r; per group the best counts over members sum to the group's frames
        one = _run(rt, x, groups, T, lens)["stats"].reshape(7, 4)
        assert one[:6, 0].tolist() == lens.tolist()
        assert [int(one[0:3, 3].sum()), int(one[3:5, 3].sum()), int(one[5, 3])] == ref["glens"].tolist()
        assert (one[:6, 1] <= one[:6, 0]).all() and (one[:6, 2] <= one[:6, 0]).all()
    assert total[6].tolist() == [77] * 4


def test_the_same_calls_give_the_same_bytes(rt):
    T, groups = 5000, [[0, 1, 2, 3, 4], [5, 6]]
    rng = np.random.default_rng(9)
    x = values(rng, 7, T)
    lens = rng.integers(1, T + 1, 7).astype(np.int32)
    weights = random_weights(rng, groups)
    configure(rt, groups, fr.MEAN, 0.5, 0.5, weights)
    outs = []
    for _ in range(3):
        got = _run(rt, x, groups, T, lens, T + 3, 1)
        outs.append(tuple(got[k].tobytes() for k in ("fused", "glens", "labels", "best", "stats")))
    assert outs[0] == outs[1] == outs[2]


def test_each_optional_output_may_be_null(rt):
    T, groups = 700, [[0, 1, 2], [3, 4]]
    rng = np.random.default_rng(13)
    x = values(rng, 5, T)
    lens = rng.integers(1, T + 1, 5).astype(np.int32)
    flags = np.array([1, 0, 2, 0, 0], np.uint8)
    for mode in MODES:
        configure(rt, groups, mode, 0.5, 0.5)
        ref = fr.fuse_ref(x, groups, mode, 0.5, 0.5, lens, flags=flags)
        for kw in ({}, {"labels": False}, {"best": False}, {"stats": False}, {"labels": False, "best": False, "stats": False}):
            _check(_run(rt, x, groups, T, lens, **kw), ref, T, what=(mode, kw), **kw)
        _check(_run(rt, x, groups, T, lens, flags=flags), ref, T, flags=True, what=(mode, "flags"))


def _pick(rt, best_dev, ld_b, tab_bytes, total, max_cuts, out_table=True, pick=True):
    lib, ctx = rt.lib, rt.ctx
    d_tab = torch.from_numpy(tab_bytes.copy()).to(DEV)
    d_total = torch.tensor([total], dtype=torch.int32, device=DEV)
    d_out = torch.full(((max_cuts + 1) * 32,), CANARY, dtype=torch.uint8, device=DEV)
    d_pick = torch.full(((max_cuts + 1) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    code = lib.uvad_fuse_pick(ctx, best_dev.data_ptr(), ld_b, d_tab.data_ptr(), d_total.data_ptr(), max_cuts,
                              d_out.data_ptr() if out_table else None, d_pick.data_ptr() if pick else None, None)
    assert code == 0, lib.uvad_last_error(ctx)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(cr.CUT_DTYPE), d_pick.cpu().numpy().view(np.int32)


def test_pick_borders(rt):
    T = 2300
    groups = [[4, 0, 2], [1, 3]]
    rng = np.random.default_rng(17)
    best = np.zeros((2, T), np.uint8)
    best[0] = rng.integers(0, 3, T)
    best[1] = rng.integers(0, 2, T)
    best[0, 100:164] = 2                                         # a cut of exactly one ballot word
    best[0, 1000:1060] = np.tile([0, 1], 30)                     # a tie between positions 0 and 1: the lowest wins
    best[1, 0:3] = [1, 0, 1]
    cuts = [(0, 0, 100, 64), (0, 1, 1000, 60), (0, 2, 1020, 1030), (0, 3, 2100, 200), (0, 4, 63, 2), (0, 5, 500, 0), (1, 0, 0, 3),
            (1, 1, 1023, 2), (1, 2, 64, 64), (7, 0, 5, 5), (-1, 0, 5, 5), (1, 3, 2299, 1)]
    tab = np.zeros(len(cuts) + 2, cr.CUT_DTYPE)
    for i, (g, k, f, n) in enumerate(cuts):
        tab[i] = (g, k, f, n, f * 160, n * 160 + 240)
    tab[len(cuts):] = (0, 99, 0, T, 0, 1)                        # past the total: never looked at
    configure(rt, groups, fr.MAX)
    d_best = torch.from_numpy(best).to(DEV)
    want_tab, want_pick = fr.pick_ref(best, groups, [tuple(int(v) for v in r) for r in tab[:len(cuts)].tolist()])
    assert want_pick[0] == 2 and want_pick[1] == 0 and want_pick[5] == 0 and want_pick[9] == -1 and want_pick[10] == -1
    raw = tab.view(np.uint8)
    for max_cuts, kw in ((len(cuts) + 2, {}), (5, {}), (len(cuts) + 2, {"out_table": False}), (len(cuts) + 2, {"pick": False}), (0, {})):
        m = min(len(cuts), max_cuts)
        out, pick = _pick(rt, d_best, T, raw, len(cuts), max_cuts, **kw)
        if kw.get("out_table", True):
            assert [tuple(int(v) for v in r) for r in out[:m].tolist()] == want_tab[:m], (max_cuts, kw)
            assert (out[m:].view(np.uint8) == CANARY).all()
        else:
            assert (out.view(np.uint8) == CANARY).all()
        if kw.get("pick", True):
            assert pick[:m].tolist() == want_pick[:m] and (pick[m:].view(np.uint8) == CANARY).all(), (max_cuts, kw)
        else:
            assert (pick.view(np.uint8) == CANARY).all()
    # positions past 63: a group of 200 members
    big = [list(range(200))]
    configure(rt, big, fr.MAX)
    b2 = rng.integers(0, 200, (1, 700)).astype(np.uint8)
    b2[0, 10:300:2] = 131
    b2[0, 400:700:3] = 67
    t2 = np.zeros(3, cr.CUT_DTYPE)
    t2[0], t2[1], t2[2] = (0, 0, 0, 350, 0, 0), (0, 1, 390, 310, 0, 0), (0, 2, 300, 64, 0, 0)
    wt, wp = fr.pick_ref(b2, big, [tuple(int(v) for v in r) for r in t2.tolist()])
    out, pick = _pick(rt, torch.from_numpy(b2).to(DEV), 700, t2.view(np.uint8), 3, 3)
    assert wp[:2] == [131, 67] and pick[:3].tolist() == wp and [tuple(int(v) for v in r) for r in out[:3].tolist()] == wt


def test_one_captured_graph_of_fuse_table_pick_gather(rt):
    Cn, F, T, hop, tail = 3, 4, 900, 160, 240
    S = T * hop + tail
    groups = [[f * Cn + c for c in range(Cn)] for f in range(F)]
    cfg = dict(pad=3, max_len=70, min_len=2, hop=hop, lead=0, tail=tail)
    st = rt.fuse_open(groups, mode="max", threshold=0.5)
    ct = rt.cuts_open(**cfg)
    B = F * Cn
    s_x = torch.zeros((B, T), dtype=torch.float32, device=DEV)
    s_len = torch.full((B,), T, dtype=torch.int32, device=DEV)
    s_pcm = torch.zeros((B, S), dtype=torch.int16, device=DEV)
    fused, glens, labels, best, _ = rt.fuse(s_x, lengths=s_len, state=st)                # sizes the buffers
    rt.cuts_table(labels, lengths=glens, S=S, cuts=ct)
    rt.fuse_pick(best, ct)
    rt.cuts_gather(s_pcm, ct, "samples", table=ct["pick_table"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # one stream; a synchronisation or allocation in the calls would fail here
        fused, glens, labels, best, stats = rt.fuse(s_x, lengths=s_len, state=st)
        table, _, total = rt.cuts_table(labels, lengths=glens, S=S, cuts=ct)
        ptab, pick = rt.fuse_pick(best, ct)
        batch, out_len = rt.cuts_gather(s_pcm, ct, "samples", table=ptab)
    rng = np.random.default_rng(23)
    for rep in range(3):
        x = np.zeros((B, T), np.float32)
        for r in range(B):                                       # smooth-ish rows: runs of speech at different levels per channel
            for _ in range(6):
                s = int(rng.integers(0, T - 40))
                x[r, s:s + int(rng.integers(5, 120))] = VALUES[int(rng.integers(2, 5))]
        lens = rng.integers(T // 2, T + 1, B).astype(np.int32)
        pcm = rng.integers(-32768, 32768, (B, S)).astype(np.int16)
        s_x.copy_(torch.from_numpy(x).to(DEV))
        s_len.copy_(torch.from_numpy(lens).to(DEV))
        s_pcm.copy_(torch.from_numpy(pcm).to(DEV))
        rt.fuse_reset_stats(st)
        graph.replay()
        torch.cuda.synchronize()
        ref = fr.fuse_ref(x, groups, fr.MAX, 0.5, 0.5, lens)
        lab = np.zeros((F, T), np.uint8)
        for g in range(F):
            lab[g, :ref["glens"][g]] = ref["labels"][g, :ref["glens"][g]]
        want, _ = cr.table(lab, ref["glens"], None, S, tuple(cfg.values()))
        n = len(want)
        assert n > 4 and int(total.cpu()[0]) == n
        wt, wp = fr.pick_ref(ref["best"], groups, [tuple(int(v) for v in r) for r in want.tolist()])
        assert len(set(wp)) > 1                                  # more than one channel is picked
        got_tab = ptab[:n].cpu().numpy().view(cr.CUT_DTYPE).reshape(-1)
        assert [tuple(int(v) for v in r) for r in got_tab.tolist()] == wt and pick[:n].cpu().tolist() == wp
        ld_out = batch.shape[1]
        wb, wl = np.zeros((n, ld_out), np.int16), np.zeros(n, np.int32)
        cr.gather(pcm, np.array(wt, cr.CUT_DTYPE), "samples", ld_out, wb, wl)
        assert batch[:n].cpu().numpy().tobytes() == wb.tobytes() and out_len[:n].cpu().numpy().tolist() == wl.tolist()
        assert stats.cpu().numpy().view(np.uint64).tobytes() == ref["stats"].tobytes()


def test_composition_with_binarize_scoring_and_the_union(rt):
    T, groups = 1200, [[0, 1], [2, 3, 4]]
    rng = np.random.default_rng(29)
    x = np.clip(np.cumsum(rng.standard_normal((5, T)) * 0.08, axis=1) + 0.5, 0, 1).astype(np.float32)
    lens = np.array([T, 1100, 900, T, 1000], np.int32)
    st = rt.fuse_open(groups, mode="mean", threshold=0.5)
    fused, glens, _, _, _ = rt.fuse(torch.from_numpy(x).to(DEV), lengths=lens, state=st)
    ref = fr.fuse_ref(x, groups, fr.MEAN, 0.5, 0.5, lens)
    d_ref = torch.from_numpy(ref["fused"]).to(DEV)
    bcfg = dict(onset=0.6, offset=0.4, min_on=5, min_off=7, pad_on=1, pad_off=2)
    a = rt.binarize(fused, lengths=glens, **bcfg)
    b = rt.binarize(d_ref, lengths=ref["glens"], **bcfg)
    gl = ref["glens"]
    for g in range(2):
        assert a[0][g, :gl[g]].cpu().numpy().tobytes() == b[0][g, :gl[g]].cpu().numpy().tobytes()
    assert a[2].cpu().tolist() == b[2].cpu().tolist() and sum(a[2].cpu().tolist()) > 0
    gt = torch.from_numpy((rng.random((2, T)) < 0.5).astype(np.uint8)).to(DEV)
    reads = []
    for p, n in ((fused, glens), (d_ref, ref["glens"])):
        sc = rt.score_open(points=((0.5, 1), (0.3, 5)))
        rt.score_step(sc, p, gt, lengths=n)
        assert rt.score_read(sc)["valid"] == int(gl.sum())
        reads.append(sc["totals"].cpu().numpy().tobytes())
    assert reads[0] == reads[1]
    # MAX at threshold = decide = 0.5 without NaN: the fused labels are the OR of the members' own threshold labels -- what
    # get_binary_tensor gives on the joined interval lists of the channels
    configure(rt, groups, fr.MAX, 0.5, 0.5)
    got = _run(rt, x, groups, T, lens)
    for g, rows in enumerate(groups):
        union = np.zeros(T, np.uint8)
        for r in rows:
            union[:lens[r]] |= (x[r, :lens[r]] >= 0.5).astype(np.uint8)
        assert got["labels"][g, :gl[g]].tolist() == union[:gl[g]].tolist()


def test_host_layer(rt):
    T, groups = 640, [[0, 2], [1, 3, 4]]
    rng = np.random.default_rng(37)
    x = values(rng, 5, T, nan=0.0)
    lens = np.array([600, T, 640, 100, 333], np.int32)
    weights = [[1.0, 3.0], [0.0, 1.0, 1.0]]
    for mode, m in (("max", fr.MAX), ("mean", fr.MEAN), ("vote", fr.VOTE)):
        st = rt.fuse_open(groups, mode=mode, threshold=0.5, weights=weights)
        ref = fr.fuse_ref(x, groups, m, 0.5, 0.5, lens, weights)
        for call in range(2):
            fused, glens, labels, best, stats = rt.fuse(torch.from_numpy(x).to(DEV), lengths=lens, state=st)
        assert glens.cpu().tolist() == ref["glens"].tolist()
        for g in range(2):
            L = ref["glens"][g]
            assert fused[g, :L].cpu().numpy().tobytes() == ref["fused"][g, :L].tobytes()
            assert labels[g, :L].cpu().numpy().tobytes() == ref["labels"][g, :L].tobytes()
            assert best[g, :L].cpu().numpy().tobytes() == ref["best"][g, :L].tobytes()
        read = rt.fuse_read(st)
        assert [len(g) for g in read] == [2, 3]
        flat = [m_ for g in read for m_ in g]
        assert [[d["valid"], d["speech"], d["agree"], d["best"]] for d in flat] == (2 * ref["stats"]).tolist()
    ct = rt.cuts_open(pad=2, max_len=50, min_len=0, hop=160, lead=0, tail=240)
    rt.cuts_table(labels, lengths=glens, cuts=ct)
    ptab, pick = rt.fuse_pick(best, ct)
    tab = rt.cuts_read(ct)
    wt, wp = fr.pick_ref(ref["best"], groups, [tuple(int(v) for v in r) for r in tab.tolist()])
    assert len(tab) > 2 and pick[:len(tab)].cpu().tolist() == wp
    assert [tuple(int(v) for v in r) for r in ptab[:len(tab)].cpu().numpy().view(cr.CUT_DTYPE).reshape(-1).tolist()] == wt
    with pytest.raises(ValueError):
        rt.fuse(torch.zeros((3, 8), device=DEV), state=st)       # the groups name row 4


def _ulaw_file(tmp_path, name, channels, seed, samples=88000):
    import ingest_ref
    import test_gpu_ingest as gi
    raw = gi._source("ulaw", (1, samples, channels), seed=seed)[0]                    # 11 s at 8 kHz
    p = str(tmp_path / name)
    ingest_ref.write_wav(p, raw, 7, 8000)
    return p


def test_predict_vad_fuses_the_channels_of_a_file(tmp_path):
    import test_gpu_ingest as gi
    from uvad_amd.postprocess import median_filter
    from uvad_amd.scripts import _write_wav_int16, predict_vad
    p = _ulaw_file(tmp_path, "array.wav", 3, 41)
    cfg = gi._predict_cfg([p], "all")
    per = predict_vad(**cfg)                                                           # what the parent commit returns
    assert [r["recording_id"] for r in per] == ["array.wav-ch0", "array.wav-ch1", "array.wav-ch2"] and "channel_stats" not in per[0]
    x = np.stack([r["probs"] for r in per])
    for mode, m in (("max", fr.MAX), ("mean", fr.MEAN)):
        cfg.fuse = {"mode": mode}
        (one,) = predict_vad(**cfg)
        ref = fr.fuse_ref(x, [[0, 1, 2]], m, 0.5, 0.5)
        assert one["recording_id"] == "array.wav" and one["channels"] == 3 and one["num_frames"] == x.shape[1]
        assert one["probs"].tobytes() == ref["fused"][0].tobytes()
        lab = median_filter(torch.from_numpy(ref["fused"]).to(DEV), window=0.01).cpu().numpy().astype(np.uint8)
        assert one["labels"].tobytes() == lab[0].tobytes()
        assert [[s["valid"], s["speech"], s["agree"], s["best"]] for s in one["channel_stats"]] == ref["stats"].tolist()
        assert [s["channel"] for s in one["channel_stats"]] == [0, 1, 2]
    # cuts: each from the channel that heard it best, with "channel"; the audio written is that channel's
    out = tmp_path / "cuts"
    cfg.cuts = {"buffer": 0.05, "split": True, "window": 1.5, "min": 0.1, "write_dir": str(out)}
    (one,) = predict_vad(**cfg)
    assert len(one["cuts"]) > 1 and all(set(c) == {"start", "end", "first_sample", "n_samples", "channel"} for c in one["cuts"])
    m_, rt = gi._predict_model(cfg)
    rt.ingest_configure("ulaw", 3, 8000)
    import uvad_amd.scripts as scr
    raw, _ = scr.read_audio(p)
    y = rt.ingest(torch.from_numpy(raw[None]).to(DEV)).cpu().numpy()                   # (3, 176000): the channels at 16 kHz
    for k, c in enumerate(one["cuts"]):
        f0, f1 = int(round(c["start"] / 0.01)), int(round(c["end"] / 0.01))
        (_, picks) = fr.pick_ref(ref["best"], [[0, 1, 2]], [(0, k, f0, f1 - f0, 0, 0)])
        assert c["channel"] == picks[0], k
        want = tmp_path / "want.wav"
        _write_wav_int16(str(want), y[c["channel"], c["first_sample"]:c["first_sample"] + c["n_samples"]], 16000)
        assert (out / f"array.wav_{k:04d}.wav").read_bytes() == want.read_bytes(), k
    assert len({c["channel"] for c in one["cuts"]}) > 1
    cfg.input.channels = "first"
    with pytest.raises(ValueError, match="channels = 'all'"):
        predict_vad(**cfg)
    cfg.input.channels = "all"
    cfg.fuse = {"mode": "max", "groups": [[0, 1]]}
    with pytest.raises(ValueError, match="groups"):
        predict_vad(**cfg)


def test_test_vad_scores_the_fused_row_of_a_two_channel_file(tmp_path):
    import test_gpu_ingest as gi
    from uvad_amd.postprocess import supervision_frames
    from uvad_amd.scripts import predict_vad
    from uvad_amd.scripts import test_vad as run_test
    p = _ulaw_file(tmp_path, "call2.wav", 2, 43)
    sups = [(0.0, 1.2), (1.0, 2.503), (4.0, 7.0), (9.5, 10.999)]
    lab = tmp_path / "call2.txt"
    lab.write_text("".join(f"{a}\t{b}\tSPC\n" for a, b in sups))
    cfg = gi._predict_cfg([p], "all")
    cfg.input.labels = [str(lab)]
    with pytest.raises(ValueError, match="one recording per file"):
        run_test(**cfg)                                                                # without fuse: refused, as before
    cfg.fuse = {"mode": "mean", "threshold": 0.5}
    got = run_test(**cfg)
    (pred,) = predict_vad(**cfg)
    n = pred["num_frames"]
    gt = np.zeros(n, np.uint8)
    for s, e in supervision_frames(sups, 11.0, frame_shift=0.01, geometry="fbank", num_frames=n):
        gt[max(s, 0):max(e, 0)] = 1
    fa = float(((pred["labels"] == 1) & (gt == 0)).sum()) / n
    md = float(((pred["labels"] == 0) & (gt == 1)).sum()) / n
    (rec,) = got["recordings"]
    assert rec["recording_id"] == "call2.wav" and rec["false_alarm"] == fa and rec["missed_detection"] == md
    assert got["detection_error_rate"] == fa + md and 0 < gt.sum() < n


@pytest.mark.parametrize("route", ["ragged", "sliding", "binarize"])
def test_predict_vad_fuse_on_the_other_routes(tmp_path, route):
    """The fused row is built from the channels' probabilities of the same route: whole recordings in a ragged batch, overlapping
    windows aggregated on the device, and (on the disjoint route) uvad_binarize in place of median + runs."""
    import test_gpu_ingest as gi
    from uvad_amd.scripts import predict_vad
    p = _ulaw_file(tmp_path, "array.wav", 3, 47)
    cfg = gi._predict_cfg([p], "all")
    if route == "ragged":
        cfg.window_seconds = None
        cfg.ragged_batches = True
    elif route == "sliding":
        cfg.hop_seconds = 2.5
    else:
        cfg.binarize = {"onset": 0.55, "offset": 0.45, "min_duration_on": 0.05, "min_duration_off": 0.08, "pad_onset": 0.02, "pad_offset": 0.03}
    per = predict_vad(**cfg)
    assert len(per) == 3 and len({r["num_frames"] for r in per}) == 1
    x = np.stack([r["probs"] for r in per])
    cfg.fuse = {"mode": "vote", "threshold": 0.5}
    (one,) = predict_vad(**cfg)
    ref = fr.fuse_ref(x, [[0, 1, 2]], fr.VOTE, 0.5, 0.5)
    assert one["recording_id"] == "array.wav" and one["num_frames"] == x.shape[1] > 0
    assert one["probs"].tobytes() == ref["fused"][0].tobytes()
    assert [[s["valid"], s["speech"], s["agree"], s["best"]] for s in one["channel_stats"]] == ref["stats"].tolist()
    assert all(0.0 <= a < b <= 11.0 for a, b in one["intervals"])
    if route == "binarize":                                      # the decision is uvad_binarize on the fused row
        import binarize_ref as br
        from uvad_amd.postprocess import binarize_config
        q = br.cfg(**binarize_config(**cfg.binarize, frame_shift=0.01))
        iv = br.row(ref["fused"][0], x.shape[1], q)
        assert one["labels"].tobytes() == br.labels_of(iv, x.shape[1]).tobytes()
