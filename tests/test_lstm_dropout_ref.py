"""The dropout restatement (tests/lstm_dropout_ref.py) on its own: Philox4x32-10 against known answers, the threshold and scale rules, the
chained forward / backward pass against torch in float64, and the statistics of the mask."""
import numpy as np
import pytest
import torch

import lstm_dropout_ref as DR
import lstm_train_ref as R


def test_philox_known_answers():
    ka = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
          ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
          ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
          ((7, 0x10003, 2, 0), (0x5EED, 0), (653133243, 3376001206, 1837702570, 3649793147))]
    for ctr, key, want in ka:
        assert tuple(int(v) for v in DR.philox4x32_10(ctr, key)) == want, ctr
    # the coordinates of include/uvad.h: frame 7, layer 1, columns 12 .. 15, draw 2, seed 0x5EED
    w = DR.words(0x5EED, 2, 1, 8, 16)
    assert tuple(int(v) for v in w[7, 12:16]) == ka[3][2]


def test_threshold_scale_and_p_zero():
    assert DR.threshold(0.5) == 0x80000000 and DR.threshold(np.float32(0.3)) == 1288490240 and DR.threshold(0.0) == 0
    assert DR.threshold(np.nextafter(np.float32(1), np.float32(0))) == 2 ** 32 - 256
    assert DR.scale(0.0) == np.float32(1.0) and DR.scale(0.5) == np.float32(2.0)
    assert DR.scale(np.float32(0.3)) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))
    assert DR.mask(0x5EED, 0, 0, 95, 128, 0.0).all()
    x = np.random.default_rng(0).standard_normal((5, 8)).astype(np.float32)
    x[0, 0], x[1, 1] = -0.0, np.nan
    assert DR.apply_f32(x, 1, 2, 3, 0.0).tobytes() == x.tobytes()                # every element kept, scale 1: the same bits


@pytest.mark.parametrize("H,dirs,layers,lens", [(64, 2, 3, [9, 0, 4, 9, 1]), (64, 1, 2, [0, 9, 5, 1, 9])])
@pytest.mark.parametrize("p", [0.5, 0.3])
def test_restatement_equals_torch_float64(H, dirs, layers, lens, p):
    Din, B, T = 16, 5, 9
    params, x, dy = R.seeded(7 + layers, Din, H, dirs, layers, 0, B, T, scale=2.0)
    a = DR.forward_backward(params, x, dy, H, dirs, layers, 0, lens, seed=0x5EED, draw=3, p=p)
    b = DR.torch_forward_backward(params, x, dy, H, dirs, layers, 0, lens, seed=0x5EED, draw=3, p=p, dtype=torch.float64)
    assert list(a["grads"]) == [k for k, _ in R.keys(Din, H, dirs, layers, 0)]
    for name, u, v in [("y", a["y"], b["y"]), ("grad_in", a["grad_in"], b["grad_in"])] + [(k, a["grads"][k], b["grads"][k]) for k in a["grads"]]:
        assert np.abs(u - v).max() <= 1e-12 * max(1.0, np.abs(v).max()), name
    assert not a["y"][~a["valid"]].any() and not a["grad_in"][~a["valid"]].any()
    # the mask matters: without it the result is another one
    c = R.forward_backward(params, x, dy, H, dirs, layers, 0, lens)
    assert np.abs(c["y"] - a["y"]).max() > 1e-3


def test_keep_fractions():
    for p, want in ((0.5, 0.5), (np.float32(0.3), 0.7)):
        for layer in (0, 1):
            for draw in (0, 1):
                f = DR.mask(0x5EED, draw, layer, 95, 128, p).mean()
                assert abs(f - want) <= 0.02, (p, layer, draw, f)


def test_masks_of_other_coordinates_differ():
    """Two independent masks at p = 0.5 differ in half their elements (12160 of them: sigma 0.0045): more than a quarter is 55 sigma away."""
    base = DR.mask(0x5EED, 0, 0, 95, 128, 0.5)
    for other in (DR.mask(0x5EED, 1, 0, 95, 128, 0.5), DR.mask(0x5EED, 1 << 32, 0, 95, 128, 0.5), DR.mask(0x5EED, 0, 1, 95, 128, 0.5),
                  DR.mask(0x5EEE, 0, 0, 95, 128, 0.5), DR.mask(0x5EED | 1 << 32, 0, 0, 95, 128, 0.5)):
        assert (base != other).mean() > 0.25
    assert np.array_equal(base, DR.mask(0x5EED, 0, 0, 95, 128, 0.5))
    # a frame's mask does not depend on how many frames there are, nor a column group's on the width
    assert np.array_equal(base[:10], DR.mask(0x5EED, 0, 0, 10, 128, 0.5)) and np.array_equal(base[:, :64], DR.mask(0x5EED, 0, 0, 95, 64, 0.5))
