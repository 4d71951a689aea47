"""The sampler's definitions (include/uvad.h, restated in tests/sampler_ref.py) checked on the CPU: the epoch permutation is a bijection and
unbiased, drop_last visits L distinct windows, and the two label rules equal postprocess.supervision_frames away from rounding edges."""
import numpy as np
import pytest

import sampler_ref as S


@pytest.mark.parametrize("N", [1, 2, 3, 5, 16, 17, 255, 256, 257, 4097, 65537])
def test_perm_is_a_bijection(N):
    for seed, d, e in ((42, 0, 0), (0xDEADBEEF12345678, 3, (1 << 32) + 5)):
        v = S.perm_all(N, seed, d, e)
        assert np.array_equal(np.sort(v), np.arange(N))
        for p in {0, N // 2, N - 1}:
            assert S.perm(N, seed, d, e, p) == v[p]              # the scalar walk is the vectorised one
    assert np.array_equal(S.perm_all(N, 42, 0, 7, shuffle=False), np.arange(N))


@pytest.mark.parametrize("N, lo, hi", [(5, 700, 900), (8, 400, 600)])
def test_perm_position_value_counts(N, lo, hi):
    """4000 epochs at seed 42: every (position, value) count lies inside the stated range (expected 4000 / N)."""
    counts = np.zeros((N, N), np.int64)
    np.add.at(counts, (np.tile(np.arange(N), 4000), S.perm_all(N, 42, 0, np.arange(4000)).reshape(-1)), 1)
    assert lo <= counts.min() and counts.max() <= hi, (counts.min(), counts.max())


def test_perm_domain_has_at_least_eight_bits():
    assert S.perm_params(2) == (8, 4, 15) and S.perm_params(256) == (8, 4, 15) and S.perm_params(257) == (10, 5, 31)
    assert S.perm_params(4097) == (14, 7, 127) and S.perm_params(65537) == (18, 9, 511) and S.perm_params((1 << 31) - 1) == (32, 16, 65535)


def _sampler(lengths, sups, W, geometry, **kw):
    frames = S.frames_fbank if geometry == S.FBANK else S.frames_sincnet
    pcm = np.arange(sum(lengths), dtype=np.float32)
    return S.Sampler(pcm, lengths, sups, W, kw.pop("min_keep", 0), geometry, frames, **kw)


def test_drop_last_epochs_visit_L_distinct_windows():
    W, B = 100, 4
    sm = _sampler([W * 11], [[]], W, S.FBANK, drop_last=True, batch=B, seed=9)         # N = 11, L = 8
    assert sm.N[0] == 11 and sm.L[0] == 8
    seen = []
    for _ in range(6):                                                                 # three epochs of two steps
        seen.append(sm.step(B)["plan"])
    plan = np.concatenate(seen)
    for e in range(3):
        rows = plan[8 * e:8 * e + 8]
        assert (rows[:, 1] == e).all() and np.array_equal(rows[:, 2], np.arange(8)) and len(set(rows[:, 3])) == 8
        assert set(rows[:, 3]) == set(S.perm_all(11, 9, 0, e)[:8])                     # the permutation's last N - L are skipped
    assert sm.cursor[0] == 24 and sm.draws == 6


def test_window_table_keeps_strictly_longer_tails_and_groups_by_dataset():
    W = 100
    win, first = S.window_table([2 * W + 30, 2 * W + 31, 29, W, W - 1, W + 1], W, 30, rec_set=[1, 0, 0, 1, 0, 1], D=2)
    assert first.tolist() == [0, 4, 8]             # a tail of exactly min_keep goes, one sample more stays; 29 samples give no window
    assert win.tolist() == [[1, 0, 100], [1, 100, 100], [1, 200, 31], [4, 0, 99], [0, 0, 100], [0, 100, 100], [3, 0, 100], [5, 0, 100]]


def test_cum_table():
    assert S.cum_table([1.0]) == [1 << 32] and S.cum_table([1, 2, 5]) == [1 << 29, 3 << 29, 1 << 32]


def test_fbank_rule_equals_supervision_frames():
    from uvad_amd.postprocess import supervision_frames
    W, hop, shift = 16000, 160, 0.01
    ks = [(0, 3), (2, 2), (5, 40), (37, 99), (98, 99)]
    times = [((a + 0.5) * shift, (b + 0.5) * shift) for a, b in ks]                    # away from every rounding edge
    for s, e in times:
        sup = [[(int(round(s * 16000)), int(round(e * 16000)))]]
        sm = _sampler([W], sup, W, S.FBANK, shuffle=False)
        got = sm.step(1)["labels"][0]
        st, et = supervision_frames([(s, e)], W / 16000, frame_shift=shift, geometry="fbank")[0]
        want = np.zeros(sm.T, np.uint8)
        want[st:et] = 1
        assert np.array_equal(got, want), (s, e)


def test_sincnet_rule_equals_supervision_frames():
    from uvad_amd.postprocess import supervision_frames
    W = 16000
    T = S.frames_sincnet(W)
    for a, b in [(0, 5000), (100, 700), (495, 497), (496, 2000), (497, 16000), (3000, 15999), (0, 16000), (766, 767), (8000, 8000)]:
        sm = _sampler([W], [[(a, b)]], W, S.SINCNET, shuffle=False)
        got = sm.step(1)["labels"][0]
        want = np.zeros(T, np.uint8)
        if b > a:
            st, et = supervision_frames([(a / 16000, b / 16000)], W / 16000, geometry="sincnet", num_frames=T)[0]
            want[st:et] = 1
        assert np.array_equal(got, want), (a, b)


def test_weighted_draws_follow_the_weights():
    sm = _sampler([300, 500, 900], [[], [], []], 100, S.FBANK, rec_set=[0, 1, 2], weights=(1, 2, 5), seed=3)
    ds = np.concatenate([sm.datasets(64, draw) for draw in range(100)])
    share = np.bincount(ds, minlength=3) / ds.size
    assert np.abs(share - np.array([1, 2, 5]) / 8).max() < 0.02, share             # 6400 draws: three sigma of the largest share is 0.018
