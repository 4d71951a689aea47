"""CPU restatement of head fine-tuning (uvad_head_train_*, include/uvad.h): the head's forward pass, the binary cross-entropy of the frames
present and the backward pass in float64; the loss gradient dz given p, operation by operation in numpy f32; one Adam step in numpy f32
with the running bias corrections 1 - beta^t.  Tensors are keyed by torch key; frames are flat (n = b T + t)."""
import numpy as np

F32 = np.float32


def keys(D0, H, L):
    """[(torch key, shape)] in state_dict order: the packed order of uvad_head_train_read."""
    out, k = [], D0
    for l in range(L):
        out += [(f"linear.{l}.weight", (H, k)), (f"linear.{l}.bias", (H,))]
        k = H
    return out + [("classifier.weight", (1, k)), ("classifier.bias", (1,))]


def pack(params, D0, H, L):
    return np.concatenate([np.asarray(params[k], F32).reshape(-1) for k, _ in keys(D0, H, L)])


def unpack(flat, D0, H, L):
    out, off = {}, 0
    for k, shape in keys(D0, H, L):
        n = int(np.prod(shape))
        out[k] = np.asarray(flat[off:off + n]).reshape(shape).copy()
        off += n
    return out


def valid_mask(B, T, lens=None):
    if lens is None:
        return np.ones((B, T), bool)
    n = np.clip(np.asarray(lens, np.int64), 0, T)
    return np.arange(T)[None, :] < n[:, None]


def leaky(v, s):
    return np.where(v > 0, v, v * s)


def forward(params, x, L, slope, valid):
    """x (B, T, D0) -> (activations a_0 .. a_L as (N, K) float64 with the rows past a length zeroed in a_0, z (N,))."""
    B, T, D0 = x.shape
    a = np.where(valid.reshape(-1, 1), x.reshape(B * T, D0), 0.0).astype(np.float64)   # a select: the rows past a length may hold anything
    acts = [a]
    for l in range(L):
        a = leaky(a @ params[f"linear.{l}.weight"].astype(np.float64).T + params[f"linear.{l}.bias"].astype(np.float64), slope)
        acts.append(a)
    z = a @ params["classifier.weight"].astype(np.float64)[0] + float(params["classifier.bias"][0])
    return acts, z


def bce_terms(p, y, w=None):
    """F.binary_cross_entropy's terms in float64 from the probabilities as given (f32 values widened exactly)."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore"):
        lp, l1p = np.maximum(np.log(p), -100.0), np.maximum(np.log(1.0 - p), -100.0)
    t = -np.where(y != 0, lp, l1p)
    return t if w is None else t * np.asarray(w, np.float64)


def dz_f64(p, y, w=None):
    p = np.asarray(p, np.float64)
    q = p * (1.0 - p)
    d = (p - (y != 0)) * (q / np.maximum(q, 1e-12))
    return d if w is None else d * np.asarray(w, np.float64)


def dz_f32(p, y, w=None):
    """The kernel's dz from its own p: p - y, q = p (1 - p), max(q, 1e-12), q / max, (p - y) * that, * w -- each one f32 rounding."""
    p = np.asarray(p, F32)
    d = (p - (np.asarray(y) != 0).astype(F32)).astype(F32)
    q = (p * (F32(1.0) - p).astype(F32)).astype(F32)
    qm = np.maximum(q, F32(1e-12))
    r = (d * (q / qm).astype(F32)).astype(F32)
    w = np.ones_like(p) if w is None else np.asarray(w, F32)
    return (w * r).astype(F32)


def backward(params, acts, dz, L, slope, valid):
    """-> ({torch key: float64 gradient of the summed loss}, grad_x (N, D0)) from dz (N,), zero past the lengths."""
    dz = np.where(valid.reshape(-1), dz, 0.0).astype(np.float64)
    g = {"classifier.weight": (dz @ acts[L])[None, :], "classifier.bias": np.array([dz.sum()])}
    d = dz[:, None] * params["classifier.weight"].astype(np.float64)
    for l in range(L, 0, -1):
        d = d * np.where(acts[l] > 0, 1.0, slope)
        g[f"linear.{l - 1}.weight"] = d.T @ acts[l - 1]
        g[f"linear.{l - 1}.bias"] = d.sum(0)
        d = d @ params[f"linear.{l - 1}.weight"].astype(np.float64)
    return g, np.where(valid.reshape(-1, 1), d, 0.0)


def loss_and_grads(params, x, L, slope, y=None, w=None, lens=None, dz=None):
    """The whole step in float64 -> dict(loss, frames, p, dz, grads, grad_x (B, T, D0)).  dz given: the caller's gradient, no loss."""
    B, T, D0 = x.shape
    valid = valid_mask(B, T, lens)
    acts, z = forward(params, x, L, slope, valid)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
    v = valid.reshape(-1)
    loss = 0.0
    if dz is None:
        yy = np.where(v, np.asarray(y).reshape(-1), 0)
        ww = None if w is None else np.where(v, np.asarray(w, np.float64).reshape(-1), 0.0)
        loss = float(np.where(v, bce_terms(p, yy, ww), 0.0).sum())
        dzz = dz_f64(p, yy, ww)
    else:
        dzz = np.where(v, np.asarray(dz, np.float64).reshape(-1), 0.0)
    grads, gx = backward(params, acts, dzz, L, slope, valid)
    return {"loss": loss, "frames": int(v.sum()), "p": p.reshape(B, T), "dz": np.where(v, dzz, 0.0).reshape(B, T), "grads": grads,
            "grad_x": gx.reshape(B, T, D0), "acts": acts}


def _grid(t):
    """The largest power of two (at most 1) that every element of t is a multiple of."""
    t, g = np.asarray(t, np.float64), 1.0
    while g > 2.0 ** -40 and not np.array_equal(np.round(t / g) * g, t):
        g /= 2.0
    return g


def exactness_margin(params, x, L, slope, dz, lens=None, calls=1):
    """For the controlled-operand tier -> (big, grid): the largest sum of |terms| over every sum the step forms (forward, both backward
    products, the bias sums; the accumulated ones `calls` times over) and the finest grid any of their terms lies on (a product of
    multiples of 2^-a and 2^-b is a multiple of 2^-(a+b)).  With big < 2^20 and grid >= 2^-4 every partial sum in ANY order is a
    multiple of 2^-4 below 2^20, so every f32 sum is exact whatever its order."""
    r = loss_and_grads(params, x, L, slope, lens=lens, dz=dz)
    acts = r["acts"]
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    big, grid = 0.0, 1.0
    for l in range(L):
        W, b = P[f"linear.{l}.weight"], P[f"linear.{l}.bias"]
        big = max(big, float((np.abs(acts[l]) @ np.abs(W).T + np.abs(b)).max()))
        grid = min(grid, _grid(acts[l]) * _grid(W), _grid(b))
    wc = P["classifier.weight"]
    dzz = r["dz"].reshape(-1)
    big = max(big, calls * float((np.abs(dzz) @ np.abs(acts[L])).max()), calls * float(np.abs(dzz).sum()))
    grid = min(grid, _grid(dzz) * _grid(acts[L]), _grid(dzz))
    d = dzz[:, None] * wc
    for l in range(L, 0, -1):
        d = d * np.where(acts[l] > 0, 1.0, slope)
        W = P[f"linear.{l - 1}.weight"]
        big = max(big, calls * float((np.abs(d).T @ np.abs(acts[l - 1])).max()), calls * float(np.abs(d).sum(0).max()), float((np.abs(d) @ np.abs(W)).max()))
        grid = min(grid, _grid(d) * _grid(acts[l - 1]), _grid(d), _grid(d) * _grid(W))
        d = d @ W
    grid = min(grid, _grid(d))
    return big, grid


def adam_init(P):
    return {"m": np.zeros(P, F32), "v": np.zeros(P, F32), "t": 0, "bc1": F32(0.0), "bc2": F32(0.0)}


def adam_step(w, acc, frames, st, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """One uvad_head_train_apply in numpy f32, every operation rounded once: g = acc / frames; m += (g - m) (1 - beta1);
    v = v beta2 + ((1 - beta2) g) g; c = 1 - beta^t advanced as c beta + (1 - beta); w -= (lr / c1) (m / (sqrt(v) / sqrt(c2) + eps)).
    frames == 0: nothing changes.  -> (w, state)."""
    if frames == 0:
        return w, st
    lr, b1, b2, eps = F32(lr), F32(beta1), F32(beta2), F32(eps)
    # 1 - beta in f64 from the double the caller wrote (the shortest decimal that rounds to the f32), rounded once: what torch hands lerp_ / addcmul_
    omb1, omb2 = F32(1.0 - float(str(b1))), F32(1.0 - float(str(b2)))
    g = (np.asarray(acc, F32) / F32(frames)).astype(F32)
    m = (st["m"] + ((g - st["m"]).astype(F32) * omb1).astype(F32)).astype(F32)
    v = ((st["v"] * b2).astype(F32) + ((omb2 * g).astype(F32) * g).astype(F32)).astype(F32)
    bc1, bc2 = F32(F32(st["bc1"] * b1) + omb1), F32(F32(st["bc2"] * b2) + omb2)   # 1 - beta^t: c <- c beta + (1 - beta)
    step_size = F32(lr / bc1)
    denom = ((np.sqrt(v).astype(F32) / np.sqrt(bc2).astype(F32)).astype(F32) + eps).astype(F32)
    w = (np.asarray(w, F32) - (step_size * (m / denom).astype(F32)).astype(F32)).astype(F32)
    return w, {"m": m, "v": v, "t": st["t"] + 1, "bc1": bc1, "bc2": bc2}
