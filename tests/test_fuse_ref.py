"""CPU checks of the numpy restatement of the channel fusion (tests/fuse_ref.py) against hand-made answers: what the GPU tests compare the
kernels with has to be right by itself."""
import numpy as np

import fuse_ref as fr

NAN = np.float32(np.nan)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_a_tie_goes_to_the_lowest_position():
    x = np.array([[0.5, 0.2, 0.9], [0.5, 0.7, 0.9], [0.1, 0.7, 0.9]], np.float32)
    r = fr.fuse_ref(x, [[0, 1, 2]], fr.MAX)
    assert r["best"][0].tolist() == [0, 1, 0] and r["fused"][0].tolist() == [0.5, np.float32(0.7), np.float32(0.9)]
    assert r["labels"][0].tolist() == [1, 1, 1]                              # 0.5 is not below 0.5
    assert r["stats"].tolist() == [[3, 2, 2, 2], [3, 3, 3, 1], [3, 2, 2, 0]]
    r = fr.fuse_ref(x, [[2, 1, 0]], fr.MAX)                                  # the same rows in another slot order: positions, not rows
    assert r["best"][0].tolist() == [1, 0, 0]


def test_nan_in_one_member():
    x = np.array([[0.9, 0.1], [NAN, 0.2], [1.0, NAN]], np.float32)
    r = fr.fuse_ref(x, [[0, 1, 2]], fr.MAX)
    assert np.isnan(r["fused"][0]).all() and r["labels"][0].tolist() == [1, 1] and r["best"][0].tolist() == [1, 2]
    # NaN counts as speech in the member's own test too: valid, speech, agree, best
    assert r["stats"].tolist() == [[2, 1, 1, 0], [2, 1, 1, 1], [2, 2, 2, 1]]
    two = np.array([[NAN], [NAN]], np.float32)
    assert fr.fuse_ref(two, [[0, 1]], fr.MAX)["best"][0].tolist() == [0]     # nothing ranks above a NaN: the first stays
    m = fr.fuse_ref(x, [[0, 1, 2]], fr.MEAN)
    assert _bits(m["fused"][0]) == [0x7fc00000, 0x7fc00000] and m["labels"][0].tolist() == [1, 1]
    v = fr.fuse_ref(x, [[0, 1, 2]], fr.VOTE)                                 # NaN votes speech
    assert v["fused"][0].tolist() == [1.0, np.float32(1.0 / 3.0)] and v["labels"][0].tolist() == [1, 0]


def test_ragged_members_and_the_group_length():
    x = np.array([[0.2, 0.4, 0.6, 0.8], [1.0, 1.0, NAN, NAN], [0.0, NAN, NAN, NAN]], np.float32)   # NaN: must not be read
    lens = [3, 2, 1]
    r = fr.fuse_ref(x, [[0, 1, 2]], fr.MEAN, lens=lens)
    assert r["glens"].tolist() == [3]                                        # the maximum, not T and not the minimum
    want = [np.float32((np.float64(np.float32(0.2)) + 1.0 + 0.0) / 3), np.float32((np.float64(np.float32(0.4)) + 1.0) / 2), np.float32(0.6)]
    assert _bits(r["fused"][0, :3]) == _bits(want) and r["fused"][0, 3] == 0 and r["best"][0, :3].tolist() == [1, 1, 0]
    assert r["stats"][:, 0].tolist() == lens
    r = fr.fuse_ref(x, [[0, 1, 2], [2]], fr.MAX, lens=[9, -4, 1])            # clamped to [0, T]; a row in two groups
    assert r["glens"].tolist() == [4, 1] and r["best"][0].tolist() == [0, 0, 0, 0] and r["stats"][1].tolist() == [0, 0, 0, 0]
    assert fr.fuse_ref(x, [[1], [0]], fr.MAX, lens=[2, 0, 0])["glens"].tolist() == [0, 2]


def test_weights():
    x = np.array([[1.0, 1.0], [0.0, 0.5], [0.5, 0.0]], np.float32)
    r = fr.fuse_ref(x, [[0, 1, 2]], fr.MEAN, weights=[[0.0, 1.0, 3.0]])
    assert r["fused"][0].tolist() == [0.375, 0.125] and r["labels"][0].tolist() == [0, 0]
    assert r["best"][0].tolist() == [0, 0]                                   # weights play no part in best: the zero-weight member wins
    # W == 0 at a frame: only the zero-weight member is valid there
    r = fr.fuse_ref(x, [[0, 1, 2]], fr.MEAN, lens=[2, 1, 1], weights=[[0.0, 1.0, 3.0]])
    assert _bits(r["fused"][0]) == _bits([0.375, 0.0]) and r["labels"][0].tolist() == [0, 0]
    r = fr.fuse_ref(x, [[0, 1, 2]], fr.VOTE, lens=[2, 1, 1], weights=[[0.0, 1.0, 3.0]])
    assert r["fused"][0].tolist() == [0.75, 0.0]
    # the accumulation is float64 in slot order: 1e8 + 1 - 1e8 keeps the 1 there, and would not in float32
    big = np.array([[1e8], [1.0], [-1e8]], np.float32)
    assert fr.fuse_ref(big, [[0, 1, 2]], fr.MEAN)["fused"][0].tolist() == [np.float32(1.0 / 3.0)]
    inf = np.array([[np.inf, np.inf], [-np.inf, 1.0]], np.float32)
    r = fr.fuse_ref(inf, [[0, 1]], fr.MEAN, weights=[[1.0, 0.0]])
    assert _bits(r["fused"][0]) == [0x7fc00000, 0x7f800000]                  # inf x 1 + (-inf) x 0 is NaN, written as the one quiet NaN


def test_vote_with_decide_a_half():
    x = np.array([[1, 0, 1, 0], [0, 0, 1, 1], [0, 0, 1, 1]], np.float32)
    two = fr.fuse_ref(x, [[0, 1]], fr.VOTE, 0.5, 0.5)
    assert two["fused"][0].tolist() == [0.5, 0.0, 1.0, 0.5] and two["labels"][0].tolist() == [1, 0, 1, 1]   # a tie of two is speech
    three = fr.fuse_ref(x, [[0, 1, 2]], fr.VOTE, 0.5, 0.5)
    assert three["labels"][0].tolist() == [0, 0, 1, 1]
    any_member = fr.fuse_ref(x, [[0, 1, 2]], fr.VOTE, 0.5, 1e-6)
    assert any_member["labels"][0].tolist() == [1, 0, 1, 1]
    assert three["stats"].tolist() == [[4, 2, 2, 3], [4, 2, 4, 1], [4, 2, 4, 0]]


def _binary_tensor(intervals, T, shift=0.01):
    """get_binary_tensor of other_vad_metrics.py on an interval list in seconds: frames [round(s / shift), round(e / shift)) set to 1."""
    y = np.zeros(T, np.uint8)
    for s, e in intervals:
        y[int(round(s / shift)):int(round(e / shift))] = 1
    return y


def test_max_fusion_is_the_union_of_the_channels_interval_lists():
    T = 400
    ch = [[(0.10, 0.55), (2.00, 2.40)], [(0.50, 0.90), (3.10, 3.11)], [(1.00, 1.20), (2.30, 2.80)]]
    rows = np.stack([_binary_tensor(iv, T) for iv in ch]).astype(np.float32)
    joined = _binary_tensor([iv for c in ch for iv in c], T)
    r = fr.fuse_ref(rows, [[0, 1, 2]], fr.MAX, 0.5, 0.5)
    assert r["labels"][0].tolist() == joined.tolist() and 0 < joined.sum() < T
    r2 = fr.fuse_ref(rows, [[0, 1]], fr.MAX, 0.5, 0.5)
    assert r2["labels"][0].tolist() == _binary_tensor(ch[0] + ch[1], T).tolist()


def test_pick():
    groups = [[4, 0, 2], [1, 3]]
    best = np.zeros((2, 200), np.uint8)
    best[0, 10:20] = [0, 1, 0, 1, 2, 2, 1, 0, 2, 9]                          # 3 : 3 : 3 and a byte that is no position
    best[0, 100:130] = 2
    best[1, 0:3] = [1, 0, 1]
    table = [(0, 0, 10, 10, 1600, 1840), (0, 1, 100, 30, 16000, 5040), (0, 2, 95, 11, 0, 0), (0, 3, 50, 0, 8000, 0), (1, 0, 0, 3, 0, 720),
             (2, 0, 0, 5, 0, 0), (-1, 0, 0, 5, 0, 0)]
    out, picks = fr.pick_ref(best, groups, table)
    assert picks == [0, 2, 2, 0, 1, -1, -1]                                  # the tie to the lowest; 6 : 5 for position 2; 0 frames -> 0
    assert [o[0] for o in out] == [4, 2, 2, 4, 3, 2, -1] and [o[1:] for o in out] == [t[1:] for t in table]
