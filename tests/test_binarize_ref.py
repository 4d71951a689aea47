"""The restatement of the hysteresis decisions (tests/binarize_ref.py) itself, without a GPU: against the threshold's runs, against
postprocess.merged_runs, on hand-written rows at each rule's boundary, and against postprocess.hysteresis_runs on random rows."""
import numpy as np
import pytest

import binarize_ref as br


def _stretches(rng, T, levels=(0.1, 0.5, 0.9), longest=40):
    """T probabilities in stretches of random length around the LO, MID and HI levels."""
    p, t = np.empty(T, np.float32), 0
    while t < T:
        n = int(rng.integers(1, longest + 1))
        p[t:t + n] = levels[int(rng.integers(0, len(levels)))] + rng.uniform(-0.05, 0.05)
        t += n
    return p


def test_equal_thresholds_and_zeros_are_the_runs_of_the_threshold():
    rng = np.random.default_rng(1)
    for T in (1, 2, 63, 64, 65, 500):
        for onset in (0.5, 0.3, 0.93):
            p = rng.random(T).astype(np.float32)
            p[rng.integers(0, T)] = np.float32(onset)              # a probability at the threshold is speech
            want = br.runs_of((p >= np.float32(onset)).tolist())
            assert br.row(p, T, br.cfg(onset)) == want
            assert br.row(p, T // 2, br.cfg(onset)) == br.runs_of((p[:T // 2] >= np.float32(onset)).tolist())


@pytest.mark.parametrize("P", [0, 1, 3, 17])
@pytest.mark.parametrize("min_off", [0, 1])
def test_symmetric_padding_is_merged_runs(P, min_off):
    from uvad_amd.postprocess import merged_runs
    rng = np.random.default_rng(10 + P)
    for T in (1, 64, 257, 1000):
        p = _stretches(rng, T, levels=(0.1, 0.9), longest=2 * P + 4)
        lab = (p >= np.float32(0.5)).astype(np.uint8)
        assert br.row(p, T, br.cfg(0.5, 0.5, 0, min_off, P, P)) == merged_runs(lab, P)


def _row(spec, T):
    """spec: [(start, stop, value)] over a row of 0.5 (MID) -> (T,) f32."""
    p = np.full(T, 0.5, np.float32)
    for a, c, v in spec:
        p[a:c] = v
    return p


def test_hand_written_rows():
    H, L = 0.9, 0.1
    q = lambda **kw: br.cfg(0.7, 0.3, **kw)
    # hysteresis: MID holds the state, LO ends it, MID before any HI stays 0
    p = _row([(3, 4, H), (8, 9, L), (12, 13, H)], 16)
    assert br.row(p, 16, q()) == [(3, 8), (12, 16)]
    assert br.row(p, 10, q()) == [(3, 8)] and br.row(p, 3, q()) == [] and br.row(p, 0, q()) == []
    # fill: a pause of min_off - 1 frames is filled, one of min_off frames is not
    p = _row([(0, 20, L), (2, 4, H), (9, 11, H)], 20)               # runs [2, 4) and [9, 11): a pause of 5
    assert br.row(p, 20, q(min_off=6)) == [(2, 11)] and br.row(p, 20, q(min_off=5)) == [(2, 4), (9, 11)]
    assert br.row(p, 20, q(min_off=0)) == br.row(p, 20, q(min_off=1)) == [(2, 4), (9, 11)]
    # pad, then fill: the pause that counts is the one between the padded intervals
    assert br.row(p, 20, q(pad_on=2, pad_off=3)) == [(0, 14)]       # [0, 7) and [7, 14) touch: merged
    assert br.row(p, 20, q(pad_on=2, pad_off=2)) == [(0, 6), (7, 13)]
    assert br.row(p, 20, q(pad_on=2, pad_off=2, min_off=2)) == [(0, 13)] and br.row(p, 20, q(pad_on=2, pad_off=2, min_off=1)) == [(0, 6), (7, 13)]
    # drop: a merged interval of min_on - 1 frames goes, one of min_on frames stays; after padding and clipping
    assert br.row(p, 20, q(min_on=2)) == [(2, 4), (9, 11)] and br.row(p, 20, q(min_on=3)) == []
    assert br.row(p, 20, q(min_on=9, min_off=6)) == [(2, 11)] and br.row(p, 20, q(min_on=10, min_off=6)) == []
    assert br.row(p, 20, q(pad_on=5, min_on=4)) == [(0, 11)]                  # [0, 4) and [4, 11) touch
    # clipping at 0 and at n
    p = _row([(0, 12, L), (1, 2, H), (10, 11, H)], 12)
    assert br.row(p, 12, q(pad_on=4, pad_off=4)) == [(0, 12)]                        # [0, 6) and [6, 12) touch
    assert br.row(p, 12, q(pad_on=4, pad_off=3)) == [(0, 5), (6, 12)]
    assert br.row(p, 11, q(pad_on=0, pad_off=9)) == [(1, 11)]
    # [0, 6) and [7, 12): the second would have 6 frames too, were it not clipped at n
    assert br.row(p, 12, q(pad_on=3, pad_off=4, min_on=6)) == [(0, 6)] and br.row(p, 12, q(pad_on=3, pad_off=4, min_on=5)) == [(0, 6), (7, 12)]
    assert br.row(p, 12, q(pad_on=4, pad_off=3, min_on=6)) == [(6, 12)]           # [0, 5), clipped at 0, goes
    # drop comes after fill: two short runs that merge survive a min_on neither meets alone
    assert br.row(_row([(0, 9, L), (1, 2, H), (4, 5, H)], 9), 9, q(min_off=3, min_on=4)) == [(1, 5)]
    # NaN counts as speech
    p = _row([(0, 8, L)], 8)
    p[2] = np.nan
    assert br.row(p, 8, q()) == [(2, 3)]
    p[3:6] = 0.5
    assert br.row(p, 8, q()) == [(2, 6)]
    # labels are the union
    assert br.labels_of([(1, 3), (5, 6)], 7).tolist() == [0, 1, 1, 0, 0, 1, 0]


def test_outputs_respect_max_iv_and_lengths():
    p = np.stack([_row([(0, 20, 0.1), (2, 4, 0.9), (9, 11, 0.9), (15, 16, 0.9)], 20)] * 2)
    lab = np.full((2, 22), 7, np.uint8)
    iv = np.full((2, 2, 2), -5, np.int32)
    cn = np.full(2, -5, np.int32)
    lab2, iv2, cn2 = br.outputs(p, [20, 10], br.cfg(0.7, 0.3), 2, lab, iv, cn)
    assert cn2.tolist() == [3, 2] and iv2[0].tolist() == [[2, 4], [9, 11]] and iv2[1].tolist() == [[2, 4], [9, 10]]
    assert lab2[0, :20].sum() == 5 and lab2[0, 15] == 1 and lab2[0, 20:].tolist() == [7, 7] and lab2[1, 10:].tolist() == [7] * 12
    assert lab[0, 0] == 7 and cn[0] == -5                             # the arrays given are not written


def test_hysteresis_runs_equals_the_restatement():
    from uvad_amd.postprocess import binarize_config, hysteresis_runs
    rng = np.random.default_rng(3)
    cases = 0
    for T in (0, 1, 64, 300, 2000):
        for kw in (dict(), dict(onset=0.7, offset=0.3), dict(onset=0.7, offset=0.3, min_on=7, min_off=5, pad_on=2, pad_off=3),
                   dict(onset=0.6, offset=0.6, min_on=0, min_off=40, pad_on=0, pad_off=9), dict(onset=0.9, offset=0.1, min_on=T + 1)):
            p = _stretches(rng, T, longest=12) if T else np.zeros(0, np.float32)
            if T > 5:
                p[rng.integers(0, T, 3)] = np.nan
            q = br.cfg(**kw)
            assert hysteresis_runs(p, q._asdict()) == br.row(p, T, q), (T, kw)
            cases += 1
    assert cases == 25
    assert binarize_config(0.6, None, 0.25, 0.1, 0.03, 0.055, 0.01) == {"onset": 0.6, "offset": 0.6, "min_on": 25, "min_off": 10, "pad_on": 3, "pad_off": 6}
    assert binarize_config(0.7, 0.4, 0.25, frame_shift=270 / 16000)["min_on"] == 15
    for bad in (dict(onset=0.3, offset=0.7), dict(onset=float("nan")), dict(min_on=-1)):
        with pytest.raises(ValueError):
            hysteresis_runs([0.5], bad)
