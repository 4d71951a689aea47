"""tests/stream_ref.py against the closed form the existing streaming tests assert, and the step shapes the path tests rely on."""

import pytest

import stream_ref as sr

# the chunks of tests/test_gpu_stream_paths.py and those of the older streaming tests (parity, scale, SincNet configurations)
CHUNKS = [160, 320, 480, 560, 640, 700, 800, 80, 200, 250, 333, 1024, 1600, 4800, 20000]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_running_sum_is_the_closed_form(chunk):
    steps = max(8, 40000 // chunk)
    ks = sr.k_schedule(chunk, steps)
    assert len(ks) == steps and min(ks) >= 0
    total = 0
    for i, k in enumerate(ks):
        total += k
        n = (i + 1) * chunk
        assert total == max(0, (n + 120 - 400) // 160 + 1), (chunk, i)
        assert total == sr.frames_complete(n)


def test_other_geometries_follow_the_definition():
    for L, sh in ((400, 160), (512, 128), (320, 160), (400, 200), (256, 100)):
        n_left = (L - sh) // 2
        for n in range(0, 3000, 7):
            t = sr.frames_complete(n, L, sh)
            assert t == 0 or (t - 1) * sh - n_left + L <= n          # the last counted frame is complete
            assert t * sh - n_left + L > n                           # and the next one is not


def test_step_shapes_the_path_tests_rely_on():
    k700 = sr.k_schedule(700, 34)
    assert k700[:6] == [3, 5, 4, 4, 5, 4]
    assert 4 in k700 and 5 in k700 and set(k700) == {3, 4, 5}       # both sides of LSTM_STACK_TMAX in one session
    k640 = sr.k_schedule(640, 25)
    assert k640[0] == 3 and set(k640[1:]) == {4}
    assert set(sr.k_schedule(800, 20)) == {4, 5} and sr.k_schedule(800, 20)[0] == 4 and set(sr.k_schedule(800, 20)[1:]) == {5}
    k560 = sr.k_schedule(560, 28)
    assert set(k560[1:]) == {3, 4} and k560[0] == 2
    assert sr.k_schedule(160, 5) == [0, 1, 1, 1, 1]                 # a first step without a frame
    assert sr.k_schedule(320, 4) == [1, 2, 2, 2]
    assert sr.k_schedule(480, 4) == [2, 3, 3, 3]


def test_frames_covering_and_positions():
    assert sr.frames_covering(8000, 100) == [49, 50]                # 49 * 160 - 120 = 7720 <= 8000 < 8120; 51 * 160 - 120 = 8040
    assert sr.frames_covering(8160, 100) == [50, 51]
    assert sr.frames_covering(0, 10) == [0]
    assert sr.frames_covering(130, 10) == [0, 1]
    for s in (5, 8000, 12345):
        for t in range(100):
            lo = t * 160 - 120
            inside = lo <= s < lo + 400 or (s < 120 and lo <= -1 - s < lo + 400)
            assert (t in sr.frames_covering(s, 100)) == inside
    ks = sr.k_schedule(640, 10)
    assert sr.step_and_position(ks, 0) == (0, 0) and sr.step_and_position(ks, 2) == (0, 2) and sr.step_and_position(ks, 3) == (1, 0)
    assert sr.step_and_position(ks, 49 - 14) == (9, 0)
    with pytest.raises(ValueError):
        sr.step_and_position(ks, sum(ks))
