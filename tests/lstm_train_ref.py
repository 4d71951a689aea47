"""CPU restatement of LSTM training (uvad_lstm_train_*, include/uvad.h) in numpy float64: the forward pass of the trainable layers with
kept activations (nn.LSTM on pack_padded_sequence rows: gate order i, f, g, o, zero initial state, the backward direction starting at
len_b - 1) and the hand-written backward pass of the header, step by step.  Tensors are keyed by torch key; x is (B, T, Din)."""
import numpy as np

NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def keys(Din, H, dirs, num_layers, first_layer=0):
    """[(torch key, shape)] of the trainable tensors in state_dict order: the packed order of uvad_lstm_train_read."""
    out = []
    for k in range(first_layer, num_layers):
        K = Din if k == first_layer else H * dirs
        for d in range(dirs):
            suf = f"_l{k}" + ("_reverse" if d else "")
            out += [(f"lstm.weight_ih{suf}", (4 * H, K)), (f"lstm.weight_hh{suf}", (4 * H, H)), (f"lstm.bias_ih{suf}", (4 * H,)),
                    (f"lstm.bias_hh{suf}", (4 * H,))]
    return out


def pack(params, *shape):
    return np.concatenate([np.asarray(params[k], np.float32).reshape(-1) for k, _ in keys(*shape)])


def unpack(flat, *shape):
    out, off = {}, 0
    for k, s in keys(*shape):
        n = int(np.prod(s))
        out[k] = np.asarray(flat[off:off + n]).reshape(s).copy()
        off += n
    return out


def lengths(B, T, lens=None):
    return np.full(B, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _order(d, n):
    """The frames of a row of length n in direction d's own order."""
    return range(n) if d == 0 else range(n - 1, -1, -1)


def forward(params, x, H, dirs, num_layers, first_layer=0, lens=None):
    """-> (y (B, T, H dirs) of the top layer, +0 past the lengths; saved: per layer the input and, per direction, i f g o c h_prev (B, T, H))."""
    B, T, _ = x.shape
    n = lengths(B, T, lens)
    valid = np.arange(T)[None, :] < n[:, None]
    inp = np.where(valid[..., None], np.asarray(x, np.float64), 0.0)      # a select: the frames past a length may hold anything
    saved = []
    for k in range(first_layer, num_layers):
        out = np.zeros((B, T, H * dirs))
        layer = {"x": inp, "dirs": []}
        for d in range(dirs):
            suf = f"_l{k}" + ("_reverse" if d else "")
            Wih, Whh = (params[f"lstm.weight_{s}{suf}"].astype(np.float64) for s in ("ih", "hh"))
            b = params[f"lstm.bias_ih{suf}"].astype(np.float64) + params[f"lstm.bias_hh{suf}"].astype(np.float64)
            keep = {s: np.zeros((B, T, H)) for s in ("i", "f", "g", "o", "c", "hp")}
            for r in range(B):
                h, c = np.zeros(H), np.zeros(H)
                for t in _order(d, int(n[r])):
                    pre = Wih @ inp[r, t] + Whh @ h + b
                    i, f, g, o = _sig(pre[:H]), _sig(pre[H:2 * H]), np.tanh(pre[2 * H:3 * H]), _sig(pre[3 * H:])
                    keep["hp"][r, t] = h
                    c = f * c + i * g
                    h = o * np.tanh(c)
                    for s, v in (("i", i), ("f", f), ("g", g), ("o", o), ("c", c)):
                        keep[s][r, t] = v
                    out[r, t, d * H:(d + 1) * H] = h
            layer["dirs"].append(keep)
        saved.append(layer)
        inp = out
    return inp, {"layers": saved, "n": n, "valid": valid}


def backward(params, saved, dy, H, dirs, num_layers, first_layer=0):
    """dy (B, T, H dirs): the gradient of the summed loss at the top layer's output (frames past a length are not read)
    -> ({torch key: float64 gradient}, grad_in (B, T, Din), +0 past the lengths)."""
    n, valid = saved["n"], saved["valid"]
    B, T = valid.shape
    d_out = np.where(valid[..., None], np.asarray(dy, np.float64), 0.0)
    grads = {}
    for li in range(num_layers - first_layer - 1, -1, -1):
        k, layer = first_layer + li, saved["layers"][li]
        x = layer["x"]
        d_in = np.zeros_like(x)
        for d in range(dirs):
            suf = f"_l{k}" + ("_reverse" if d else "")
            Wih, Whh = (params[f"lstm.weight_{s}{suf}"].astype(np.float64) for s in ("ih", "hh"))
            kp = layer["dirs"][d]
            dpre = np.zeros((B, T, 4 * H))
            for r in range(B):
                frames = list(_order(d, int(n[r])))
                dh_rec, dc_rec = np.zeros(H), np.zeros(H)
                for pos in range(len(frames) - 1, -1, -1):                # reverse time in the direction's own order
                    t = frames[pos]
                    i, f, g, o, c = (kp[s][r, t] for s in ("i", "f", "g", "o", "c"))
                    c_prev = kp["c"][r, frames[pos - 1]] if pos else np.zeros(H)
                    tc = np.tanh(c)
                    dh = d_out[r, t, d * H:(d + 1) * H] + dh_rec
                    do = dh * tc
                    dc = dh * o * (1.0 - tc * tc) + dc_rec
                    di, dg, df = dc * g, dc * i, dc * c_prev
                    p = np.concatenate([di * i * (1.0 - i), df * f * (1.0 - f), dg * (1.0 - g * g), do * o * (1.0 - o)])
                    dpre[r, t] = p
                    dc_rec = dc * f
                    dh_rec = p @ Whh
            flat = dpre.reshape(B * T, 4 * H)
            grads[f"lstm.weight_ih{suf}"] = flat.T @ x.reshape(B * T, -1)
            grads[f"lstm.weight_hh{suf}"] = flat.T @ kp["hp"].reshape(B * T, H)
            grads[f"lstm.bias_ih{suf}"] = flat.sum(0)
            grads[f"lstm.bias_hh{suf}"] = flat.sum(0)
            d_in += dpre @ Wih
        d_out = np.where(valid[..., None], d_in, 0.0)
    return grads, d_out


def forward_backward(params, x, dy, H, dirs, num_layers, first_layer=0, lens=None):
    y, saved = forward(params, x, H, dirs, num_layers, first_layer, lens)
    grads, gin = backward(params, saved, dy, H, dirs, num_layers, first_layer)
    return {"y": y, "grads": grads, "grad_in": gin, "valid": saved["valid"], "saved": saved}


def torch_forward_backward(params, x, dy, H, dirs, num_layers, first_layer=0, lens=None, dtype=None):
    """The same through torch.nn.LSTM with pack_padded_sequence(enforce_sorted=False) and autograd on the CPU, in `dtype`
    -> dict(y, grads, grad_in) of numpy arrays.  Rows of length 0 (which pack_padded_sequence refuses) are left out and come back as zeros."""
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    dtype = dtype or torch.float64
    B, T, Din = x.shape
    n = lengths(B, T, lens)
    rows = np.nonzero(n > 0)[0]
    nl = num_layers - first_layer
    lstm = torch.nn.LSTM(Din, H, nl, batch_first=True, bidirectional=dirs == 2).to(dtype)
    with torch.no_grad():
        for key, _ in keys(Din, H, dirs, num_layers, first_layer):
            name, k = key[len("lstm."):].rsplit("_l", 1)
            rev = k.endswith("_reverse")
            li = int(k.replace("_reverse", "")) - first_layer
            getattr(lstm, f"{name}_l{li}" + ("_reverse" if rev else "")).copy_(torch.tensor(np.asarray(params[key]), dtype=dtype))
    y, gin = np.zeros((B, T, H * dirs)), np.zeros((B, T, Din))
    grads = {key: np.zeros(s) for key, s in keys(Din, H, dirs, num_layers, first_layer)}
    if len(rows):
        valid = np.arange(T)[None, :] < n[:, None]
        xt = torch.tensor(np.where(valid[..., None], x, 0.0)[rows], dtype=dtype, requires_grad=True)
        out, _ = lstm(pack_padded_sequence(xt, torch.tensor(n[rows]), batch_first=True, enforce_sorted=False))
        out, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
        out.backward(torch.tensor(np.where(valid[..., None], dy, 0.0)[rows], dtype=dtype))
        y[rows], gin[rows] = out.detach().numpy(), xt.grad.numpy()
        for key in grads:
            name, k = key[len("lstm."):].rsplit("_l", 1)
            li = int(k.replace("_reverse", "")) - first_layer
            grads[key] = getattr(lstm, f"{name}_l{li}" + ("_reverse" if k.endswith("_reverse") else "")).grad.numpy().astype(np.float64)
    return {"y": y, "grads": grads, "grad_in": gin}


def seeded(seed, Din, H, dirs, num_layers, first_layer, B, T, scale=1.0):
    """A seeded problem: weights uniform in +-scale / sqrt(H) (nn.LSTM's initialisation times scale), x and dy standard normal."""
    rng = np.random.default_rng(seed)
    params = {k: (rng.uniform(-1, 1, s) * scale / np.sqrt(H)).astype(np.float32) for k, s in keys(Din, H, dirs, num_layers, first_layer)}
    x = rng.standard_normal((B, T, Din)).astype(np.float32)
    dy = rng.standard_normal((B, T, H * dirs)).astype(np.float32)
    return params, x, dy
