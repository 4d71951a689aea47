"""float64 restatement of SincNet training as include/uvad.h states it for uvad_sincnet_train_*: the forward pass with kept pooled values,
winners and statistics, and the backward pass step by step (numpy), plus the same network through torch.nn.functional with a differentiable
restatement of ParamSincFB.filters() (autograd's result on the reference module is the defining semantic), packing helpers and the decision
margins the GPU tests choose their seeds by.  Reference geometry: 80 x 251 sinc bank at stride 10, Conv1d(80, 60, 5), Conv1d(60, 60, 5)."""
import math

import numpy as np
import torch
import torch.nn.functional as F
from numpy.lib.stride_tricks import sliding_window_view

NF, KS, STRIDE, C2, K2, C3, K3 = 80, 251, 10, 60, 5, 60, 5
SLOPE, EPS = 0.01, 1e-5
MIN_LOW, MIN_BAND, RATE = 50.0, 50.0, 16000.0
# (stage, key, shape) in state_dict order
TENSORS = [(0, "wav_norm1d.weight", (1,)), (0, "wav_norm1d.bias", (1,)), (0, "conv1d.0.filterbank.low_hz_", (NF // 2, 1)),
           (0, "conv1d.0.filterbank.band_hz_", (NF // 2, 1)), (1, "conv1d.1.weight", (C2, NF, K2)), (1, "conv1d.1.bias", (C2,)),
           (2, "conv1d.2.weight", (C3, C2, K3)), (2, "conv1d.2.bias", (C3,)), (0, "norm1d.0.weight", (NF,)), (0, "norm1d.0.bias", (NF,)),
           (1, "norm1d.1.weight", (C2,)), (1, "norm1d.1.bias", (C2,)), (2, "norm1d.2.weight", (C3,)), (2, "norm1d.2.bias", (C3,))]


def keys(first_stage=0):
    return [(k, shape) for s, k, shape in TENSORS if s >= first_stage]


def pack(params, first_stage=0, dtype=np.float32):
    return np.concatenate([np.asarray(params[k], dtype).reshape(-1) for k, _ in keys(first_stage)])


def unpack(flat, first_stage=0):
    out, off = {}, 0
    for k, shape in keys(first_stage):
        n = int(np.prod(shape))
        out[k] = np.asarray(flat[off:off + n]).reshape(shape).copy()
        off += n
    assert off == len(flat)
    return out


def num_frames(S):
    n = (S - KS) // STRIDE + 1
    for _ in range(2):
        n = n // 3 - 4
    return n // 3


def buffers():
    """ParamSincFB's f32 buffers window_ [125] and n_ [125], as the module builds them."""
    half = KS // 2
    window = torch.from_numpy(np.hamming(KS)[:half]).float()
    n_ = 2 * math.pi * (torch.arange(-half, 0.0).view(1, -1) / RATE)
    return window.numpy().copy(), n_.numpy().reshape(-1).copy()


def init_params(seed, gamma_range=(0.5, 1.5)):
    """torch's own initialisation of the reference modules (f32 numpy), the norms' gamma uniform in gamma_range, beta in [-0.2, 0.2]."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    c1, c2 = torch.nn.Conv1d(NF, C2, K2), torch.nn.Conv1d(C2, C3, K3)
    to_mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)
    to_hz = lambda mel: 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    hz = to_hz(np.linspace(to_mel(30.0), to_mel(RATE / 2 - (MIN_LOW + MIN_BAND)), NF // 2 + 1, dtype="float32")).astype(np.float32)
    u = lambda n, lo, hi: (lo + (hi - lo) * torch.rand(n, generator=g)).numpy().astype(np.float32)
    p = {"wav_norm1d.weight": u(1, *gamma_range), "wav_norm1d.bias": u(1, -0.2, 0.2),
         "conv1d.0.filterbank.low_hz_": hz[:-1].reshape(-1, 1).copy(), "conv1d.0.filterbank.band_hz_": np.diff(hz).reshape(-1, 1).copy(),
         "conv1d.1.weight": c1.weight.detach().numpy().copy(), "conv1d.1.bias": c1.bias.detach().numpy().copy(),
         "conv1d.2.weight": c2.weight.detach().numpy().copy(), "conv1d.2.bias": c2.bias.detach().numpy().copy()}
    for s, n in ((0, NF), (1, C2), (2, C3)):
        p[f"norm1d.{s}.weight"], p[f"norm1d.{s}.bias"] = u(n, *gamma_range), u(n, -0.2, 0.2)
    return p


# ---------------------------------------------------------------- the bank
def _edges(low_p, band_p):
    lp, bp = np.asarray(low_p, np.float64).reshape(-1), np.asarray(band_p, np.float64).reshape(-1)
    low = MIN_LOW + np.abs(lp)
    raw = low + MIN_BAND + np.abs(bp)
    return lp, bp, low, raw, np.clip(raw, MIN_LOW, RATE / 2)


def filters(low_p, band_p):
    """ParamSincFB.filters() in float64 from the f32 parameters and the f32 buffers: [NF][KS]."""
    win, n = (b.astype(np.float64) for b in buffers())
    _, _, low, _, high = _edges(low_p, band_p)
    band = (high - low)[:, None]
    fl, fh = low[:, None] * n[None, :], high[:, None] * n[None, :]
    cl = ((np.sin(fh) - np.sin(fl)) / (n / 2)) * win
    sl = ((np.cos(fl) - np.cos(fh)) / (n / 2)) * win
    cos = np.concatenate([cl, 2 * band, cl[:, ::-1]], 1) / (2 * band)
    sin = np.concatenate([sl, np.zeros_like(band), -sl[:, ::-1]], 1) / (2 * band)
    return np.concatenate([cos, sin], 0)


def filters_backward(dF, low_p, band_p):
    """d low_hz_, d band_hz_ [NF / 2] from dF [NF][KS]: the chain rule through filters()."""
    win, n = (b.astype(np.float64) for b in buffers())
    lp, bp, low, raw, high = _edges(low_p, band_p)
    half, cut = KS // 2, NF // 2
    band = (high - low)[:, None]
    gc = dF[:cut, :half] + dF[:cut, :half:-1]
    gs = dF[cut:, :half] - dF[cut:, :half:-1]
    fl, fh = low[:, None] * n, high[:, None] * n
    dH = ((win / band) * (gc * np.cos(fh) + gs * np.sin(fh))).sum(1)
    dL = -((win / band) * (gc * np.cos(fl) + gs * np.sin(fl))).sum(1)
    Q = ((gc * (np.sin(fh) - np.sin(fl)) + gs * (np.cos(fl) - np.cos(fh))) * win / (n * band)).sum(1)
    dB = -Q / band[:, 0]
    dhigh, dlow = dH + dB, dL - dB
    draw = np.where((raw >= MIN_LOW) & (raw <= RATE / 2), dhigh, 0.0)
    dlow = dlow + draw
    return dlow * np.sign(lp), draw * np.sign(bp)


# ---------------------------------------------------------------- forward / backward, float64
def _conv(a, W, stride):
    win = sliding_window_view(a, W.shape[2], axis=1)[:, ::stride]       # [Cin][L][Kw]
    return np.einsum("oik,ilk->ol", W, win, optimize=True), win


def forward(params, wav, bank=None):
    """wav [B][S] -> feats [B][T][C3] (float64) and the cache the backward pass reads."""
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    wav = np.asarray(wav, np.float64)
    Fb = filters(params["conv1d.0.filterbank.low_hz_"], params["conv1d.0.filterbank.band_hz_"]) if bank is None else np.asarray(bank, np.float64)
    g, b0 = P["wav_norm1d.weight"][0], P["wav_norm1d.bias"][0]
    rows = []
    for x in wav:
        mean, var = x.mean(), x.var()
        xhat0 = (x - mean) / np.sqrt(var + EPS)
        a = (g * xhat0 + b0)[None, :]
        c = {"xhat0": xhat0, "stages": []}
        for s in range(3):
            W = Fb[:, None, :] if s == 0 else P[f"conv1d.{s}.weight"]
            u, win = _conv(a, W, STRIDE if s == 0 else 1)
            if s > 0:
                u = u + P[f"conv1d.{s}.bias"][:, None]
            upre = u
            if s == 0:
                u = np.abs(u)
            Lp = u.shape[1] // 3
            u3 = u[:, :3 * Lp].reshape(u.shape[0], Lp, 3)
            w = u3.argmax(2)                                            # the lowest index wins a tie
            p = np.take_along_axis(u3, w[..., None], 2)[..., 0]
            sign = np.sign(np.take_along_axis(upre[:, :3 * Lp].reshape(u.shape[0], Lp, 3), w[..., None], 2)[..., 0])
            mean_p, var_p = p.mean(1, keepdims=True), p.var(1, keepdims=True)
            rstd = 1.0 / np.sqrt(var_p + EPS)
            xhat = (p - mean_p) * rstd
            z = P[f"norm1d.{s}.weight"][:, None] * xhat + P[f"norm1d.{s}.bias"][:, None]
            c["stages"].append({"a_in": a, "u": u, "upre": upre, "w": w, "sign": sign, "p": p, "rstd": rstd, "xhat": xhat, "z": z, "L": u.shape[1]})
            a = np.where(z > 0, z, z * SLOPE)
        c["feats"] = a.T
        rows.append(c)
    return np.stack([c["feats"] for c in rows]), {"rows": rows, "bank": Fb}


def backward(params, cache, dfeats, first_stage=0, abs_terms=None):
    """dfeats [B][T][C3], the gradient of the summed loss -> {key: gradient} of the learning tensors, and `bias_abs`: sum |du| per
    conv1d.{1,2}.bias element (what a bias gradient's error is measured against: the gradient itself is mathematically zero)."""
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    Fb = cache["bank"]
    grads = {k: np.zeros(shape) for k, shape in keys(first_stage)}
    bias_abs = {f"conv1d.{s}.bias": np.zeros(C2 if s == 1 else C3) for s in (1, 2)}
    G, D = np.zeros((NF, KS)), np.zeros(NF)
    for c, dy in zip(cache["rows"], np.asarray(dfeats, np.float64)):
        da = dy.T
        for s in (2, 1, 0):
            if s < first_stage:
                break
            st = c["stages"][s]
            gamma = P[f"norm1d.{s}.weight"][:, None]
            dz = da * np.where(st["z"] > 0, 1.0, SLOPE)
            grads[f"norm1d.{s}.weight"] += (dz * st["xhat"]).sum(1)
            grads[f"norm1d.{s}.bias"] += dz.sum(1)
            dxhat = dz * gamma
            dp = st["rstd"] * (dxhat - dxhat.mean(1, keepdims=True) - st["xhat"] * (dxhat * st["xhat"]).mean(1, keepdims=True))
            if s == 0:
                dp = dp * st["sign"]
            C, Lp = dp.shape
            du3 = np.zeros((C, Lp, 3))
            np.put_along_axis(du3, st["w"][..., None], dp[..., None], 2)
            du = np.zeros((C, st["L"]))                                 # the positions past 3 Lp stay 0
            du[:, :3 * Lp] = du3.reshape(C, 3 * Lp)
            if s == 0:
                win = sliding_window_view(c["xhat0"], KS)[::STRIDE]     # [L][KS]
                G += du @ win
                D += du.sum(1)
                break
            W = P[f"conv1d.{s}.weight"]
            win = sliding_window_view(st["a_in"], W.shape[2], axis=1)   # [Cin][L][Kw]
            grads[f"conv1d.{s}.weight"] += np.einsum("ot,itk->oik", du, win, optimize=True)
            if abs_terms is not None:                                   # sum of the absolute terms of every weight-gradient element
                abs_terms[f"conv1d.{s}.weight"] = abs_terms.get(f"conv1d.{s}.weight", 0.0) + np.einsum("ot,itk->oik", np.abs(du), np.abs(win), optimize=True)
            grads[f"conv1d.{s}.bias"] += du.sum(1)
            bias_abs[f"conv1d.{s}.bias"] += np.abs(du).sum(1)
            da = np.zeros_like(st["a_in"])
            for k in range(W.shape[2]):
                da[:, k:k + st["L"]] += W[:, :, k].T @ du
    if first_stage == 0:
        g, b0 = P["wav_norm1d.weight"][0], P["wav_norm1d.bias"][0]
        dF = g * G + b0 * D[:, None]
        grads["wav_norm1d.weight"][0] = (Fb * G).sum()
        if abs_terms is not None:                                       # the instance norm above cancels the waveform's scale: d g is a sum that
            abs_terms["wav_norm1d.weight"] = np.abs(Fb * G).sum()       # cancels to (nearly) zero, measured against its absolute terms
        grads["wav_norm1d.bias"][0] = (D * Fb.sum(1)).sum()
        dl, db = filters_backward(dF, params["conv1d.0.filterbank.low_hz_"], params["conv1d.0.filterbank.band_hz_"])
        grads["conv1d.0.filterbank.low_hz_"][:, 0], grads["conv1d.0.filterbank.band_hz_"][:, 0] = dl, db
    return grads, bias_abs


def margins(cache):
    """Per stage the smallest relative gap of a decision of the float64 forward pass: `pool` a winner over its runner-up and `abs` (stage 0)
    the winning |u| from 0, both over max |u|; `leaky` |z| from 0 over max |z|."""
    out = []
    for s in range(3):
        pool, ab, lk, umax, zmax = np.inf, np.inf, np.inf, 0.0, 0.0
        for c in cache["rows"]:
            st = c["stages"][s]
            Lp = st["p"].shape[1]
            u3 = np.sort(st["u"][:, :3 * Lp].reshape(-1, Lp, 3), 2)
            pool, umax = min(pool, (u3[..., 2] - u3[..., 1]).min()), max(umax, np.abs(st["u"]).max())
            ab = min(ab, st["p"].min()) if s == 0 else ab
            lk, zmax = min(lk, np.abs(st["z"]).min()), max(zmax, np.abs(st["z"]).max())
        out.append({"pool": pool / umax, "abs": ab / umax if s == 0 else np.inf, "leaky": lk / zmax})
    return out


# ---------------------------------------------------------------- the same network on torch (CPU), any dtype
def torch_filters(low_p, band_p, dtype):
    win, n = (torch.from_numpy(b).to(dtype) for b in buffers())
    n = n.view(1, -1)
    low = MIN_LOW + torch.abs(low_p)
    high = torch.clamp(low + MIN_BAND + torch.abs(band_p), MIN_LOW, RATE / 2)
    band = (high - low)[:, 0]
    ft_low, ft_high = torch.matmul(low, n), torch.matmul(high, n)
    cos_left = ((torch.sin(ft_high) - torch.sin(ft_low)) / (n / 2)) * win
    cos = torch.cat([cos_left, 2 * band.view(-1, 1), torch.flip(cos_left, dims=[1])], dim=1) / (2 * band[:, None])
    sin_left = ((torch.cos(ft_low) - torch.cos(ft_high)) / (n / 2)) * win
    sin = torch.cat([sin_left, torch.zeros_like(band.view(-1, 1)), -torch.flip(sin_left, dims=[1])], dim=1) / (2 * band[:, None])
    return torch.cat([cos, sin], dim=0).view(NF, 1, KS)


def _instance_norm(x, weight, bias):
    if x.shape[2] > 1:
        return F.instance_norm(x, weight=weight, bias=bias, eps=EPS)
    # one position: F.instance_norm refuses it in training mode; the same expression written out (xhat = 0)
    xhat = (x - x.mean(2, keepdim=True)) / torch.sqrt(x.var(2, unbiased=False, keepdim=True) + EPS)
    return xhat * weight[None, :, None] + bias[None, :, None]


def torch_sincnet(T, wav):
    """The module's forward (sincnet.py:72-103) on tensors T[key]: wav [B][S] -> feats [B][T][C3] and the pre-decision tensors."""
    pre = {}
    x = F.instance_norm(wav[:, None, :], weight=T["wav_norm1d.weight"], bias=T["wav_norm1d.bias"], eps=EPS)
    for s in range(3):
        if s == 0:
            x = F.conv1d(x, torch_filters(T["conv1d.0.filterbank.low_hz_"], T["conv1d.0.filterbank.band_hz_"], wav.dtype), stride=STRIDE)
            x = torch.abs(x)
        else:
            x = F.conv1d(x, T[f"conv1d.{s}.weight"], T[f"conv1d.{s}.bias"])
        pre[f"u{s}"] = x.detach()
        x = _instance_norm(F.max_pool1d(x, 3, 3), T[f"norm1d.{s}.weight"], T[f"norm1d.{s}.bias"])
        pre[f"z{s}"] = x.detach()
        x = F.leaky_relu(x, SLOPE)
    return x.transpose(1, 2), pre


def torch_forward_backward(params, wav, dfeats, dtype=torch.float64):
    """-> feats, {key: gradient} (numpy float64) of sum(feats * dfeats), and the pre-decision tensors, all computed in `dtype`."""
    T = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items()}
    feats, pre = torch_sincnet(T, torch.tensor(np.asarray(wav), dtype=dtype))
    (feats * torch.tensor(np.asarray(dfeats), dtype=dtype)).sum().backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).double().numpy() for k, t in T.items()}
    return feats.detach().double().numpy(), grads, {k: v.double().numpy() for k, v in pre.items()}


def torch_pre(params, wav, dtype):
    """The pre-decision tensors (u0 .. u2 after |.|, z0 .. z2) of the torch forward pass in `dtype`, as float64 numpy."""
    with torch.no_grad():
        T = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
        _, pre = torch_sincnet(T, torch.tensor(np.asarray(wav), dtype=dtype))
    return {k: v.double().numpy() for k, v in pre.items()}


def make_case(B, S, seed):
    """The GPU tests' inputs: torch's initialisation with gamma in [0.5, 1.5], wav = 0.1 randn, dfeats = randn."""
    p = init_params(seed)
    g = torch.Generator().manual_seed(1000 + seed)
    wav = (0.1 * torch.randn(B, S, generator=g)).numpy().astype(np.float32)
    dfeats = torch.randn(B, num_frames(S), C3, generator=g).numpy().astype(np.float32)
    return p, wav, dfeats


def decision_clearance(params, wav):
    """-> (margins of the float64 forward pass, the f32 deviations of the pre-decision tensors, ok): ok iff every margin is at least
    8 x the largest relative deviation between torch-f32 and torch-f64 of the tensor the decision is taken on."""
    _, cache = forward(params, wav)
    m = margins(cache)
    p32, p64 = torch_pre(params, wav, torch.float32), torch_pre(params, wav, torch.float64)
    dev = {k: float(np.abs(p32[k] - p64[k]).max() / np.abs(p64[k]).max()) for k in p64}
    ok = all(m[s]["pool"] >= 8 * dev[f"u{s}"] and m[s]["abs"] >= 8 * dev[f"u{s}"] and m[s]["leaky"] >= 8 * dev[f"z{s}"] for s in range(3))
    return m, dev, ok


# ---------------------------------------------------------------- the whole chain: SincNet -> one 64-unit bidirectional LSTM layer -> a 32 / 1 head
def chain_init(seed):
    """torch's own initialisation of the LSTM layer and the head under the seed -> {model state_dict key: f32 numpy}."""
    torch.manual_seed(10_000 + seed)
    lstm, lin, cls = torch.nn.LSTM(C3, 64, 1, batch_first=True, bidirectional=True), torch.nn.Linear(128, 32), torch.nn.Linear(32, 1)
    sd = {"lstm." + k: v for k, v in lstm.state_dict().items()}
    sd.update({"linear.0.weight": lin.weight, "linear.0.bias": lin.bias, "classifier.weight": cls.weight, "classifier.bias": cls.bias})
    return {k: v.detach().numpy().copy() for k, v in sd.items()}


def chain_loop(params, rest, wav, y, steps, dtype, lr=1e-3, check=False):
    """`steps` full training steps (mean BCE over the frames, torch.optim.Adam on every tensor) in `dtype` on the CPU -> (the losses,
    how many leading steps met decision_clearance on the parameters the step started from; counted only with check)."""
    T = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items()}
    lstm, lin, cls = torch.nn.LSTM(C3, 64, 1, batch_first=True, bidirectional=True), torch.nn.Linear(128, 32), torch.nn.Linear(32, 1)
    lstm.load_state_dict({k[len("lstm."):]: torch.from_numpy(v) for k, v in rest.items() if k.startswith("lstm.")})
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(rest["linear.0.weight"])), lin.bias.copy_(torch.from_numpy(rest["linear.0.bias"]))
        cls.weight.copy_(torch.from_numpy(rest["classifier.weight"])), cls.bias.copy_(torch.from_numpy(rest["classifier.bias"]))
    lstm, lin, cls = lstm.to(dtype), lin.to(dtype), cls.to(dtype)
    opt = torch.optim.Adam(list(T.values()) + list(lstm.parameters()) + list(lin.parameters()) + list(cls.parameters()), lr=lr)
    wav_t, y_t = torch.tensor(np.asarray(wav), dtype=dtype), torch.tensor(np.asarray(y), dtype=dtype)
    losses, clear, still = [], 0, check
    for _ in range(steps):
        if still:
            still = decision_clearance({k: v.detach().numpy() for k, v in T.items()}, wav)[2]
            clear += int(still)
        opt.zero_grad(set_to_none=True)
        feats, _ = torch_sincnet(T, wav_t)
        o, _ = lstm(feats)
        p = torch.sigmoid(cls(F.leaky_relu(lin(o), SLOPE))).squeeze(-1)
        loss = F.binary_cross_entropy(p, y_t)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses), clear


def chain_case(seed, B=2, S=2071):
    p, wav, _ = make_case(B, S, seed)
    g = torch.Generator().manual_seed(2000 + seed)
    y = (torch.rand(B, num_frames(S), generator=g) < 0.5).numpy().astype(np.uint8)
    return p, chain_init(seed), wav, y
