"""CPU restatement of dropout between the trainable LSTM layers (uvad_lstm_train_set_dropout, uvad_dropout_apply, include/uvad.h): the
Philox4x32-10 mask as a pure function of (seed, draw, layer, frame, column), and the forward / backward pass of lstm_train_ref.py chained
one layer at a time with the mask applied between the layers in float64.  The torch comparator is the reference's non-monolithic forward
with the mask given: stacked one-layer nn.LSTMs on pack_padded_sequence rows, the explicit mask multiplied in under autograd."""
import numpy as np

import lstm_train_ref as R

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> 4 uint32 arrays (Salmon et al., the Random123 definition: ten rounds, the key
    bumped after each round)."""
    c = [np.asarray(v, np.uint64) & _U32 for v in counter]
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _U32, p1 >> np.uint64(32), p1 & _U32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """thr = (uint32) floor((double)p 2^32) for p given as an f32."""
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def scale(p):
    """1.0f / (1.0f - p) in IEEE f32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(seed, draw, layer, N, cols):
    """The Philox word of every (frame n, column j): counter (n, (layer << 16) | (j >> 2), draw_lo, draw_hi), key (seed_lo, seed_hi), word j & 3."""
    assert cols % 4 == 0 and 0 <= layer <= 65535
    n = np.repeat(np.arange(N, dtype=np.uint64), cols // 4)
    jq = np.tile(np.arange(cols // 4, dtype=np.uint64), N)
    out = philox4x32_10((n, (np.uint64(layer) << np.uint64(16)) | jq, draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1).reshape(N, cols)


def mask(seed, draw, layer, N, cols, p):
    """(N, cols) bool: True where the element is kept (word >= thr)."""
    return words(seed, draw, layer, N, cols) >= np.uint32(threshold(p))


def apply_f32(x, seed, draw, layer, p):
    """uvad_dropout_apply to the bit: x (rows, cols) f32 -> keep ? fl(x scale) : +0."""
    x = np.ascontiguousarray(x, np.float32)
    keep = mask(seed, draw, layer, x.shape[0], x.shape[1], p)
    with np.errstate(all="ignore"):
        return np.where(keep, x * scale(p), np.float32(0.0)).astype(np.float32)


def factors(seed, draw, H, dirs, num_layers, first_layer, B, T, p):
    """{absolute layer k: (B, T, H dirs) float64 factor (0 or scale)} for first_layer <= k < num_layers - 1."""
    s = float(scale(p))
    return {k: mask(seed, draw, k, B * T, H * dirs, p).reshape(B, T, H * dirs) * s for k in range(first_layer, num_layers - 1)}


def forward(params, x, H, dirs, num_layers, first_layer=0, lens=None, seed=0, draw=0, p=0.0):
    """-> (y of the top layer, saved).  Layer k + 1 reads the masked, scaled output of layer k; the top layer's output is never dropped."""
    B, T, _ = x.shape
    f = factors(seed, draw, H, dirs, num_layers, first_layer, B, T, p)
    inp, saved = np.asarray(x, np.float64), []
    for k in range(first_layer, num_layers):
        y, s = R.forward(params, inp, H, dirs, k + 1, k, lens)
        saved.append(s)
        inp = y * f[k] if k in f else y
    return inp, {"layers": saved, "factors": f}


def backward(params, saved, dy, H, dirs, num_layers, first_layer=0):
    """-> ({torch key: float64 gradient}, grad_in).  The dy of layer k is the masked, scaled d_in of layer k + 1, with the forward pass's mask."""
    grads, d = {}, np.asarray(dy, np.float64)
    for k in range(num_layers - 1, first_layer - 1, -1):
        g, d = R.backward(params, saved["layers"][k - first_layer], d, H, dirs, k + 1, k)
        grads.update(g)
        if k - 1 in saved["factors"]:
            d = d * saved["factors"][k - 1]
    return {key: grads[key] for key, _ in R.keys(x_width(saved), H, dirs, num_layers, first_layer)}, d


def x_width(saved):
    return saved["layers"][0]["layers"][0]["x"].shape[-1]


def forward_backward(params, x, dy, H, dirs, num_layers, first_layer=0, lens=None, seed=0, draw=0, p=0.0):
    y, saved = forward(params, x, H, dirs, num_layers, first_layer, lens, seed, draw, p)
    grads, gin = backward(params, saved, dy, H, dirs, num_layers, first_layer)
    return {"y": y, "grads": grads, "grad_in": gin, "valid": saved["layers"][0]["valid"]}


def torch_layers(params, Din, H, dirs, num_layers, first_layer, dtype):
    """The trainable layers as a list of one-layer nn.LSTMs holding `params` (the reference's non-monolithic variant)."""
    import torch
    out = []
    for k in range(first_layer, num_layers):
        m = torch.nn.LSTM(Din if k == first_layer else H * dirs, H, 1, batch_first=True, bidirectional=dirs == 2).to(dtype)
        with torch.no_grad():
            for name, prm in m.named_parameters():
                prm.copy_(torch.as_tensor(np.asarray(params["lstm." + name.replace("_l0", f"_l{k}")]), dtype=dtype))
        out.append(m)
    return out


def torch_stack(layers, x, n, factors, first_layer):
    """x (rows, T, Din) with every row's length n > 0 -> the top layer's padded output; factors[k] (rows, T, H dirs) tensors multiplied in."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    out = x
    for li, m in enumerate(layers):
        out, _ = m(pack_padded_sequence(out, n, batch_first=True, enforce_sorted=False))
        out, _ = pad_packed_sequence(out, batch_first=True, total_length=x.shape[1])
        if first_layer + li in factors:
            out = out * factors[first_layer + li]
    return out


def torch_forward_backward(params, x, dy, H, dirs, num_layers, first_layer=0, lens=None, seed=0, draw=0, p=0.0, dtype=None):
    """The same through torch on the CPU in `dtype` -> dict(y, grads, grad_in).  Rows of length 0 are left out and come back as zeros."""
    import torch
    dtype = dtype or torch.float64
    B, T, Din = x.shape
    n = R.lengths(B, T, lens)
    rows = np.nonzero(n > 0)[0]
    y, gin = np.zeros((B, T, H * dirs)), np.zeros((B, T, Din))
    grads = {key: np.zeros(s) for key, s in R.keys(Din, H, dirs, num_layers, first_layer)}
    if len(rows):
        layers = torch_layers(params, Din, H, dirs, num_layers, first_layer, dtype)
        sc = torch.tensor(float(scale(p)), dtype=dtype)
        f = {k: torch.as_tensor(mask(seed, draw, k, B * T, H * dirs, p).reshape(B, T, -1)[rows]).to(dtype) * sc
             for k in range(first_layer, num_layers - 1)}
        valid = np.arange(T)[None, :] < n[:, None]
        xt = torch.tensor(np.where(valid[..., None], x, 0.0)[rows], dtype=dtype, requires_grad=True)
        out = torch_stack(layers, xt, torch.tensor(n[rows]), f, first_layer)
        out.backward(torch.tensor(np.where(valid[..., None], dy, 0.0)[rows], dtype=dtype))
        y[rows], gin[rows] = out.detach().numpy(), xt.grad.numpy()
        for key in grads:
            name, k = key[len("lstm."):].rsplit("_l", 1)
            li = int(k.replace("_reverse", "")) - first_layer
            grads[key] = getattr(layers[li], f"{name}_l0" + ("_reverse" if k.endswith("_reverse") else "")).grad.numpy().astype(np.float64)
    return {"y": y, "grads": grads, "grad_in": gin}
