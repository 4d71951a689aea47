"""The restatement of the reverberation stage (tests/reverb_ref.py) against definitions written out plainly: the convolution as a double
loop, the threshold at prob 0 and 1, the tie rule of the delay, and the separation of its Philox stream from the mix stage's."""
import numpy as np

import mix_ref as mr
import reverb_ref as rr

SEED = 0x0123456789ABCDEF


def _brute(x, h, d):
    n, z = len(x), np.zeros(len(x), np.float64)
    for i in range(n):
        for k in range(len(h)):
            j = i + d - k
            if 0 <= j < n:
                z[i] += float(h[k]) * float(x[j])
    return z


def test_convolution_against_a_double_loop():
    rng = np.random.default_rng(1)
    for n, K in ((0, 3), (1, 1), (1, 5), (7, 1), (7, 3), (5, 9), (40, 33), (33, 40)):
        x = rng.integers(-64, 65, n).astype(np.float32)
        h = rng.integers(-8, 9, K).astype(np.float32)
        for d in sorted({0, K // 2, K - 1}):
            assert np.array_equal(rr.conv64(x, h, d), _brute(x, h, d)), (n, K, d)
            assert np.array_equal(rr.bound(x, h, d), _brute(np.abs(x), np.abs(h), d)), (n, K, d)
    assert not np.signbit(rr.conv64(np.array([-0.0, 1.0], np.float32), np.array([0.0], np.float32), 0)).any()      # a sum of zeros is +0


def test_whole_stage_against_the_double_loop():
    rng = np.random.default_rng(2)
    B, S, lens, ks = 6, 50, [50, 0, 1, 17, 49, 33], [1, 4, 20]
    first = np.r_[0, np.cumsum(ks)]
    bank = rng.integers(-8, 9, int(first[-1])).astype(np.float32)
    x = rng.integers(-64, 65, (B, S)).astype(np.int16)
    for normalize, align, max_taps in ((0, 0, 0), (0, 1, 0), (1, 1, 3), (1, 0, 0)):
        got = rr.reverb(x, lens, bank, first, 0.6, normalize, align, max_taps, SEED, 6, row0=1)
        K = rr.taps(first, max_taps)
        assert list(K) == ([1, 3, 3] if max_taps else ks)
        xf = x.astype(np.float32) / np.float32(32768.0)
        applied = got["plan"][:, 0]
        assert 0 < applied.sum() < B
        for b, n in enumerate(lens):
            assert not got["out"][b, n:].any()
            if not applied[b]:
                assert tuple(got["plan"][b]) == (0, 0, 0, rr.ONE_BITS) and np.array_equal(got["out"][b, :n], xf[b, :n])
                continue
            r, d = got["plan"][b, 1:3]
            h = bank[first[r]:first[r] + K[r]]
            assert d == (rr.delay(h) if align else 0)
            z = _brute(xf[b, :n], h, d).astype(np.float32)
            g = np.float32(1.0)
            if normalize and mr.energy(xf[b], n) != 0 and mr.energy(z, n) != 0:
                g = np.float32(np.sqrt(mr.energy(xf[b], n) / mr.energy(z, n)))
            assert got["plan"][b, 3] == g.view(np.int32) and np.array_equal(got["out"][b, :n], z * g)


def test_threshold_at_prob_zero_and_one():
    assert rr.threshold(0.0) == 0 and rr.threshold(1.0) == 1 << 32 and rr.threshold(0.5) == 1 << 31
    dly = np.array([3, 0], np.int32)
    for draw in (0, 1, (1 << 33) + 5):
        assert not rr.plan(64, 2, dly, 0.0, 1, SEED, draw)[:, 0].any()
        assert rr.plan(64, 2, dly, 1.0, 1, SEED, draw)[:, 0].all()
    p = rr.plan(512, 2, dly, 0.5, 1, SEED, 0)
    assert 200 < p[:, 0].sum() < 312 and set(p[p[:, 0] == 1, 1]) == {0, 1}
    assert (p[:, 2] == np.where(p[:, 0] == 1, dly[p[:, 1]], 0)).all() and not rr.plan(512, 2, dly, 0.5, 0, SEED, 0)[:, 2].any()
    assert rr.plan(4, 2, dly, 0.5, 1, SEED, 0, row0=3)[0].tobytes() == p[3].tobytes()      # row b of a batch = row 0 under row0 = b


def test_delay_takes_the_first_of_equal_peaks_and_never_a_nan():
    assert rr.delay([0.5, -1.0, 1.0, 0.25]) == 1 and rr.delay([np.nan, 0.5, np.nan, 0.5]) == 1
    assert rr.delay([0.0, 0.0]) == 0 and rr.delay([np.nan, np.nan]) == 0 and rr.delay([-3.0]) == 0
    assert rr.delay([0.0, 1.0, np.inf, -np.inf]) == 2
    assert list(rr.delays(np.array([0, 1, 0, 2, 0, 0, 5], np.float32), [0, 2, 7], 3)) == [1, 1]      # max_taps cuts before the search


def test_stream_is_separate_from_the_mix_stream_under_one_seed():
    rows = np.arange(256)
    for draw in (0, 7):
        own = rr.words(SEED, draw, rows)
        for k in range(64):                                          # every segment index the mix stage can use
            assert not (own == mr.words(SEED, draw, rows, k)).any()
    assert rr.WORD1 == 0x52560000 and rr.WORD1 > 63
