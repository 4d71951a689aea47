"""tests/lstm_train_ref.py, the float64 restatement the GPU tests of uvad_lstm_train_* compare against, equals torch.nn.LSTM with
pack_padded_sequence(enforce_sorted=False) and autograd in float64 on the CPU to 1e-12 of each tensor's largest magnitude: the forward
output, every parameter gradient and the input gradient, over the shapes of tests/test_gpu_lstm_train.py and ragged lengths with rows of
length 0 and 1."""
import numpy as np
import pytest

import lstm_train_ref as R

# (Din, H, dirs, num_layers, first_layer, B, T, lens)
CASES = [
    (4, 64, 1, 1, 0, 1, 1, None),
    (60, 64, 2, 1, 0, 4, 2, [2, 0, 1, 2]),
    (80, 64, 2, 2, 0, 5, 5, [5, 0, 1, 3, 9]),
    (128, 64, 2, 3, 1, 5, 5, [4, 5, -2, 1, 2]),
    (256, 128, 2, 1, 0, 5, 37, [37, 0, 1, 20, 40]),
    (60, 128, 1, 1, 0, 9, 5, [1] * 9),
    (4, 128, 1, 2, 0, 4, 37, None),
    (80, 64, 1, 1, 0, 3, 5, [0, 0, 0]),
]


@pytest.mark.parametrize("Din,H,dirs,layers,first,B,T,lens", CASES)
def test_restatement_equals_torch_float64_autograd(Din, H, dirs, layers, first, B, T, lens):
    params, x, dy = R.seeded(Din + H + B + T, Din, H, dirs, layers, first, B, T, scale=2.0)
    got = R.forward_backward(params, x, dy, H, dirs, layers, first, lens)
    want = R.torch_forward_backward(params, x, dy, H, dirs, layers, first, lens)
    pairs = [("y", got["y"], want["y"]), ("grad_in", got["grad_in"], want["grad_in"])]
    pairs += [(k, got["grads"][k], want["grads"][k]) for k, _ in R.keys(Din, H, dirs, layers, first)]
    assert len(pairs) == 2 + 4 * dirs * (layers - first)
    for name, a, b in pairs:
        assert a.shape == b.shape, name
        scale = np.abs(b).max()
        if scale == 0.0:
            assert not a.any(), name                                      # no valid frame, or no recurrent term: exactly zero on both sides
        else:
            assert np.abs(a - b).max() <= 1e-12 * scale, (name, np.abs(a - b).max() / scale)
    valid = got["valid"]
    assert not got["grad_in"][~valid].any() and not got["y"][~valid].any()    # 0 past the lengths
    n = R.lengths(B, T, lens)
    for k, _ in R.keys(Din, H, dirs, layers, first):
        if "weight_hh" in k and n.max() <= 1:
            assert not got["grads"][k].any(), k                           # every row's first step has h_prev = 0
        if "bias_hh" in k:
            assert np.array_equal(got["grads"][k], got["grads"][k.replace("bias_hh", "bias_ih")])


def test_nothing_past_a_length_is_read_and_pack_round_trips():
    Din, H, dirs, layers, first, B, T = 60, 64, 2, 2, 0, 4, 5
    lens = [5, 2, 0, 1]
    params, x, dy = R.seeded(3, Din, H, dirs, layers, first, B, T)
    a = R.forward_backward(params, x, dy, H, dirs, layers, first, lens)
    valid = a["valid"]
    xn, dn = x.copy(), dy.copy()
    xn[~valid], dn[~valid] = np.nan, np.nan
    b = R.forward_backward(params, xn, dn, H, dirs, layers, first, lens)
    assert np.array_equal(a["y"], b["y"]) and np.array_equal(a["grad_in"], b["grad_in"])
    assert all(np.array_equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
    shape = (Din, H, dirs, layers, first)
    flat = R.pack(params, *shape)
    assert flat.size == sum(int(np.prod(s)) for _, s in R.keys(*shape)) == 2 * (256 * 60 + 256 * 64 + 512) + 2 * (256 * 128 + 256 * 64 + 512)
    back = R.unpack(flat, *shape)
    assert list(back) == [k for k, _ in R.keys(*shape)] and all(np.array_equal(back[k], params[k]) for k in params)
    assert [k for k, _ in R.keys(4, 64, 2, 3, 2)] == ["lstm.weight_ih_l2", "lstm.weight_hh_l2", "lstm.bias_ih_l2", "lstm.bias_hh_l2",
                                                       "lstm.weight_ih_l2_reverse", "lstm.weight_hh_l2_reverse", "lstm.bias_ih_l2_reverse",
                                                       "lstm.bias_hh_l2_reverse"]
