"""SincNet training on the device (uvad_sincnet_train_*, include/uvad.h) against tests/sincnet_train_ref.py and torch on the CPU.

  exact structure   bits, no tolerance: two runs, a row inside a batch against the row alone, fl(gA + gB) accumulation, canaries around the
                    state, the workspace and feats, a backward call on a workspace whose header names another (B, S), first_stage = 2
                    against first_stage = 0, one frame ((1, 991): only norm1d.2.bias gets a gradient, the rest is +0), a captured graph of
                    forward -> backward -> apply; the bank within 1 f32 ulp of the float64 restatement; a silent row (the winner
                    bytes read back: index 0 at every tie); every gradient loosely (1e-3) against the restatement at every shape
  accuracy          feats and every parameter gradient: error against float64 over the float64 tensor's max-abs (conv1d.{1,2}.bias:
                    over sum |du|), max and rms, at most 4 x what torch autograd in f32 on the CPU achieves on the same inputs, pooled over
                    three seeds.  The seeds keep the float64 reference clear of every decision (|.|, pool, leaky_relu): each margin of
                    sincnet_train_ref.margins() is at least 8 x the f32 deviation of the tensor the decision is taken on; asserted on the
                    CPU before the GPU is touched.  Measured on the CPU for the seeds below (smallest margin / f32 deviation per stage):
                      (2, 2071) seeds 1, 2, 3:   pool 1.1e-5 .. 2.7e-4 / u 7.5e-7 .. 1.8e-6;  leaky 4.4e-5 .. 1.6e-3 / z 1.5e-6 .. 7.6e-6
                      (2, 4003) seeds 1, 20, 27: pool 1.1e-5 .. 2.2e-4 / u 6.3e-7 .. 1.6e-6;  leaky 1.6e-5 .. 5.0e-4 / z 1.2e-6 .. 3.3e-6
                      stage 0's winning |u| stays 3.5e-3 .. 7.6e-3 of max |u| from 0
                    (3, 8000): no seed among 0 .. 3799 meets the condition (the best reaches 6.0 x, the condition asks 8 x), so that
                    shape is in the exact-structure tier only.
  optimiser         uvad_sincnet_train_apply equals the numpy-f32 Adam restatement of tests/head_train_ref.py bit for bit; full steps of
                    SincNet -> LSTM -> head track the float64 torch loop within 4 x the deviation of torch's own f32 loop (five steps
                    for the one seed of 300 whose float64 trajectory stays clear of every decision that long, four for two more)
  commit / host     uvad_sincnet serves the committed front end in the default split-f16 form and in the exact-f32 form; other contexts untouched; VadModel("PyanNet").train_step / train_commit
"""
import ctypes as C

import numpy as np
import pytest
import torch

import head_train_ref as HR
import sincnet_train_ref as R

gpu = pytest.mark.gpu
PAD = 256
CANARY = 0xA5
SHAPES = [(1, 991), (2, 2071), (3, 8000), (2, 4003)]
SEEDS = {(2, 2071): (1, 2, 3), (2, 4003): (1, 20, 27)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _dev():
    return torch.device("cuda:0")


def _model(params, seed=3):
    """A PyanNet (one bidirectional 64-unit LSTM layer, a 32 / 1 head) whose SincNet holds `params`."""
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet(lstm={"hidden_size": 64, "num_layers": 1, "bidirectional": True, "dropout": 0.0}, linear={"hidden_size": 32, "num_layers": 1})
    m.build()
    seed_weights(m, seed, 1.0)
    sd = m.state_dict()
    with torch.no_grad():
        for k, v in params.items():
            sd["sincnet." + k].copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32)))
    return m


class Trainer:
    """The C entry points on buffers with canaries on both sides (the runtime's wrappers own plain buffers)."""

    def __init__(self, rt, first_stage=0, segment=32, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        from uvad_amd import _lib
        self.rt, self.lib, self.L = rt, rt.lib, _lib
        self.cfg = _lib.SincNetTrainCfg(lr, betas[0], betas[1], eps, segment, first_stage)
        self.first = first_stage
        self.configure()
        self.P = int(self.lib.uvad_sincnet_train_param_count(rt.ctx))
        self.nstate = int(self.lib.uvad_sincnet_train_state_bytes(rt.ctx))
        self.sbuf = torch.full((self.nstate + 2 * PAD,), CANARY, dtype=torch.uint8, device=_dev())
        self.state = self.sbuf.data_ptr() + PAD
        self.out = torch.zeros(max(self.P, 80 * 251), dtype=torch.float32, device=_dev())
        self.ws, self.bufs = {}, []
        self.rt._check(self.lib.uvad_sincnet_train_reset(rt.ctx, self.state, self.nstate, None))

    def configure(self):
        self.rt._check(self.lib.uvad_sincnet_train_configure(self.rt.ctx, C.byref(self.cfg)))

    def _ws(self, B, S, key=None, room=0):
        need = int(self.lib.uvad_sincnet_train_ws_bytes(self.rt.ctx, B, S))
        assert need > 0
        key = key or (B, S)
        if key not in self.ws:
            self.ws[key] = torch.full((need + room + 2 * PAD,), CANARY, dtype=torch.uint8, device=_dev())
        assert self.ws[key].numel() - 2 * PAD >= need
        return self.ws[key], need

    def forward(self, wav, ws_key=None, room=0):
        self.configure()
        B, S = wav.shape
        T = R.num_frames(S)
        w, need = self._ws(B, S, ws_key, room)
        fb = torch.full((B * T * 60 + 2 * PAD,), -7.0, dtype=torch.float32, device=_dev())
        self.bufs.append((fb, B * T * 60))
        self.rt._check(self.lib.uvad_sincnet_train_forward(self.rt.ctx, wav.data_ptr(), B, S, fb.data_ptr() + 4 * PAD, self.state, self.nstate,
                                                           w.data_ptr() + PAD, need, None))
        return fb[PAD:PAD + B * T * 60].view(B, T, 60)

    def backward(self, wav, dfeats, ws_key=None):
        self.configure()
        B, S = wav.shape
        w, need = self._ws(B, S, ws_key)
        self.rt._check(self.lib.uvad_sincnet_train_backward(self.rt.ctx, wav.data_ptr(), dfeats.data_ptr(), B, S, self.state, self.nstate,
                                                            w.data_ptr() + PAD, need, None))

    def apply(self):
        self.configure()
        self.rt._check(self.lib.uvad_sincnet_train_apply(self.rt.ctx, self.state, self.nstate, None))

    def read(self, which):
        self.configure()
        self.rt._check(self.lib.uvad_sincnet_train_read(self.rt.ctx, self.state, self.nstate, which, self.out.data_ptr(), None))
        a = self.out.cpu().numpy().copy()
        if which == self.L.SINCNET_TRAIN_FILTERS:
            return a[:80 * 251].reshape(80, 251)
        if which != self.L.HEAD_TRAIN_SCALARS:
            return a[:self.P]
        w = a[:8]
        return {"frames": int(w[2:4].view(np.uint64)[0]), "t": int(w[4:6].view(np.uint64)[0]), "bc1": w[6], "bc2": w[7]}

    def grad(self):
        return self.read(self.L.HEAD_TRAIN_GRAD)

    def state_bytes(self):
        return bytes(self.sbuf[PAD:PAD + self.nstate].cpu().numpy())

    def canaries_intact(self):
        ok = all(bool((b[:PAD] == CANARY).all()) and bool((b[PAD + n:] == CANARY).all())
                 for b, n in [(self.sbuf, self.nstate)] + [(w, w.numel() - 2 * PAD) for w in self.ws.values()])
        return ok and all(bool((b[:PAD] == -7.0).all()) and bool((b[PAD + n:] == -7.0).all()) for b, n in self.bufs)


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run(rt, wav, dfeats, first_stage=0, segment=32):
    t = Trainer(rt, first_stage, segment)
    feats = t.forward(wav).clone()
    t.backward(wav, dfeats)
    return t, feats, t.grad()


# ------------------------------------------------------------------------------------------------ exact structure
@gpu
@pytest.mark.parametrize("B,S", SHAPES)
def test_bits_two_runs_row_alone_accumulation_canaries_and_the_header_guard(B, S):
    seed = SEEDS.get((B, S), (1,))[0]
    p, wav_h, df_h = R.make_case(B, S, seed)
    rt = _model(p).runtime(_dev())
    wav, df = _to(wav_h), _to(df_h)
    t1, f1, g1 = _run(rt, wav, df)
    t2, f2, g2 = _run(rt, wav, df)
    assert bytes(f1.cpu().numpy()) == bytes(f2.cpu().numpy()) and np.array_equal(_bits(g1), _bits(g2)) and t1.state_bytes() == t2.state_bytes()
    assert t1.read(t1.L.HEAD_TRAIN_SCALARS)["frames"] == B * R.num_frames(S)
    assert np.isfinite(f1.cpu().numpy()).all() and np.isfinite(g1).all()
    # sanity against the float64 restatement (the accuracy tier holds the bound): feats to 1e-4 of max-abs
    ref_f, cache = R.forward(p, wav_h)
    assert np.abs(f1.cpu().numpy() - ref_f).max() <= 1e-4 * np.abs(ref_f).max()
    g = R.unpack(g1)
    terms = {}
    ref_g, bias_abs = R.backward(p, cache, df_h, abs_terms=terms)
    if R.num_frames(S) > 1:
        # every gradient against the restatement, loosely (1e-3 of max-abs; the biases over sum |du|): this tolerates an f32 decision that
        # differs from float64's at a near-tie -- one term among thousands -- where the accuracy tier's seeds rule that out.  At (3, 8000),
        # where no seed meets the clearance condition, this is the check of the backward pass against a reference.  wav_norm1d.weight is
        # measured over the sum of its absolute terms here: the instance norm above the bank cancels the waveform's scale, so that gradient
        # is a sum that cancels to nearly zero, as the conv biases' (torch-f32 itself is 4e-4 of its value off at (3, 8000))
        for k, _ in R.keys():
            scale = bias_abs[k].max() if k in bias_abs else terms[k] if k == "wav_norm1d.weight" else np.abs(ref_g[k]).max()
            e = float(np.abs(g[k] - ref_g[k]).max() / scale)
            print(f"({B}, {S}) {k:32s} error over scale {e:.3e}")
            assert e <= 1e-3, (k, e)
    if R.num_frames(S) == 1:
        # the last norm sees one position, xhat = 0: only norm1d.2.bias gets a gradient, everything else is exactly +0
        assert np.abs(g["norm1d.2.bias"] - ref_g["norm1d.2.bias"]).max() <= 1e-5 * np.abs(ref_g["norm1d.2.bias"]).max()
        for k, _ in R.keys():
            if k != "norm1d.2.bias":
                assert not _bits(g[k]).any(), k
    if B > 1:
        # a row inside a batch is that row alone
        ta = Trainer(rt)
        fa = ta.forward(wav[1:2].contiguous())
        assert bytes(fa.cpu().numpy()) == bytes(f1[1:2].cpu().numpy())
        assert ta.canaries_intact()
    # fl(gA + gB) over two micro-batches
    p2, wav2_h, df2_h = R.make_case(B, S, seed + 100)
    wav2, df2 = _to(wav2_h), _to(df2_h)
    _, _, gB = _run(rt, wav2, df2)
    tab = Trainer(rt)
    tab.forward(wav), tab.backward(wav, df), tab.forward(wav2), tab.backward(wav2, df2)
    assert np.array_equal(_bits(tab.grad()), _bits(g1 + gB))
    assert tab.read(tab.L.HEAD_TRAIN_SCALARS)["frames"] == 2 * B * R.num_frames(S)
    # a backward call on a workspace whose header names another (B, S) changes no byte of the state
    tg = Trainer(rt)
    tg.forward(wav, ws_key="shared", room=1 << 20)
    tg.backward(wav, df, ws_key="shared")
    before = tg.state_bytes()
    wav3 = _to(np.concatenate([wav_h, wav_h[:, :10]], 1))
    tg.forward(wav3, ws_key="shared")                                   # the header now names (B, S + 10)
    tg.backward(wav, df, ws_key="shared")
    torch.cuda.synchronize()
    assert tg.state_bytes() == before
    for t in (t1, t2, tab, tg):
        assert t.canaries_intact()
    rt.close()


@gpu
def test_first_stage_2_learns_stage_2_only_and_serves_the_same_feats():
    B, S = 2, 2071
    p, wav_h, df_h = R.make_case(B, S, 1)
    rt = _model(p).runtime(_dev())
    wav, df = _to(wav_h), _to(df_h)
    t0, f0, g0 = _run(rt, wav, df, 0)
    t2, f2, g2 = _run(rt, wav, df, 2)
    assert t2.P == 18180 and t0.P == 42602
    assert bytes(f0.cpu().numpy()) == bytes(f2.cpu().numpy())
    u0, u2 = R.unpack(g0, 0), R.unpack(g2, 2)
    assert list(u2) == ["conv1d.2.weight", "conv1d.2.bias", "norm1d.2.weight", "norm1d.2.bias"]
    for k in u2:
        assert np.array_equal(_bits(u2[k]), _bits(u0[k])), k
    t1, f1, g1 = _run(rt, wav, df, 1)
    u1 = R.unpack(g1, 1)
    assert t1.P == 42360 and bytes(f1.cpu().numpy()) == bytes(f0.cpu().numpy()) and all(np.array_equal(_bits(u1[k]), _bits(u0[k])) for k in u1)
    assert t0.canaries_intact() and t1.canaries_intact() and t2.canaries_intact()
    rt.close()


@gpu
def test_the_bank_is_within_one_ulp_of_the_float64_restatement():
    p, wav_h, _ = R.make_case(1, 991, 4)
    p["conv1d.0.filterbank.band_hz_"][39, 0] = 9000.0          # into the clamp
    p["conv1d.0.filterbank.low_hz_"][0, 0] = 0.0
    p["conv1d.0.filterbank.band_hz_"][7, 0] *= -1.0
    rt = _model(p).runtime(_dev())
    t = Trainer(rt)
    t.forward(_to(wav_h))
    bank = t.read(t.L.SINCNET_TRAIN_FILTERS)
    want = R.filters(p["conv1d.0.filterbank.low_hz_"], p["conv1d.0.filterbank.band_hz_"]).astype(np.float32)
    ulp = np.spacing(np.abs(want))
    worst = float((np.abs(bank.astype(np.float64) - want.astype(np.float64)) / ulp).max())
    print(f"bank: worst deviation {worst:.2f} ulp, {int((bank != want).sum())} of {bank.size} elements differ")
    assert worst <= 1.0
    rt.close()


def _winner_bytes(t, B, S):
    """The workspace's winner bytes per stage, [B][C][Lp] (the layout of uvad_internal.h: header and fold record 512 bytes, row statistics,
    then per stage pooled values, winner bytes, mean / rstd, gradient buffer; every part 256-byte aligned)."""
    al = lambda v: (v + 255) // 256 * 256
    L = (S - 251) // 10 + 1
    off, out = 512 + al(16 * B), []
    w = t.ws[(B, S)][PAD:]
    for C_, k in ((80, None), (60, 5), (60, 5)):
        L = L if k is None else L - k + 1
        Lp = L // 3
        n = B * C_ * Lp
        off += al(4 * n)
        out.append(w[off:off + n].cpu().numpy().reshape(B, C_, Lp))
        off += al(n) + al(8 * B * C_) + al(4 * n)              # first_stage 0: every stage has a gradient buffer
        L = Lp
    return out


@gpu
def test_a_silent_row_gives_finite_feats_and_gradients():
    """All-zero samples: every stage sees constant rows, so every pool is a three-way tie and every xhat is 0.  The winner bytes read back
    from the workspace are index 0 everywhere, as the restatement's argmax.  Compared to the restatement: feats; norm1d.2.bias (the one
    sum without cancellation); conv1d.2.weight and conv1d.2.bias over the sum of their absolute terms -- du = rstd (dxhat - mean) is
    formed from f32 values whose rounding is 2^-24 of terms of its own size, and the contraction adds sqrt(K) 2^-24 of sum |terms|, so
    1e-5 of sum |terms| is generous.  norm1d.s.weight is exactly +0 on the device (xhat is exactly 0: the f32 mean of equal values is the
    value).  Below stage 2 each norm's backward multiplies the residue of the stage above by rstd = 1 / sqrt(eps) = 316 (float64 gives
    1e-11 where f32 gives 1e-2 of the terms), and below stage 0's |.| the sign of a residue decides: those gradients, mathematically
    zero, are checked to be finite."""
    B, S = 1, 2071
    p, _, df_h = R.make_case(B, S, 2)
    wav_h = np.zeros((B, S), np.float32)
    rt = _model(p).runtime(_dev())
    t, f, g = _run(rt, _to(wav_h), _to(df_h))
    ref_f, cache = R.forward(p, wav_h)
    terms = {}
    ref_g, bias_abs = R.backward(p, cache, df_h, abs_terms=terms)
    assert np.isfinite(f.cpu().numpy()).all() and np.isfinite(g).all()
    assert np.abs(f.cpu().numpy() - ref_f).max() <= 1e-5 * np.abs(ref_f).max()
    for s, idx in enumerate(_winner_bytes(t, B, S)):
        want = np.stack([c["stages"][s]["w"] for c in cache["rows"]])
        assert idx.shape == want.shape and not (idx & 3).any() and not want.any(), s
    got = R.unpack(g)
    k = "norm1d.2.bias"
    assert np.abs(got[k] - ref_g[k]).max() <= 1e-5 * np.abs(ref_g[k]).max()
    for k, scale in (("conv1d.2.weight", terms["conv1d.2.weight"]), ("conv1d.2.bias", bias_abs["conv1d.2.bias"])):
        e = float((np.abs(got[k] - ref_g[k]) / scale).max())
        print(f"silent row {k}: error over sum |terms| {e:.3e}")
        assert e <= 1e-5, (k, e)
    for s in range(3):
        assert not _bits(got[f"norm1d.{s}.weight"]).any(), s
    assert t.canaries_intact()
    rt.close()


@gpu
def test_a_captured_graph_of_the_whole_step_replays_to_the_eager_bytes():
    B, S = 2, 2071
    p, _, _ = R.make_case(B, S, 1)
    rt = _model(p).runtime(_dev())
    batches = [tuple(_to(a) for a in R.make_case(B, S, 40 + k)[1:]) for k in range(3)]

    def step(h, wav, df):
        f = rt.sincnet_train_forward(h, wav)
        rt.sincnet_train_backward(h, wav, df)
        rt.sincnet_train_apply(h)
        return f
    e = rt.sincnet_train_open(lr=1e-3, segment=32)
    for wav, df in batches:
        fe = step(e, wav, df).clone()
    g = rt.sincnet_train_open(lr=1e-3, segment=32)
    swav, sdf = torch.zeros_like(batches[0][0]), torch.zeros_like(batches[0][1])
    rt.sincnet_train_forward(g, swav)                                             # sizes the workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                 # one stream; a synchronisation or allocation would fail here
        fg = step(g, swav, sdf)
    assert rt.sincnet_train_read(g)["step"] == 0                                  # captured, not run
    for wav, df in batches:
        swav.copy_(wav), sdf.copy_(df)
        graph.replay()
    torch.cuda.synchronize()
    assert bytes(e["state"].cpu().numpy()) == bytes(g["state"].cpu().numpy())
    assert bytes(fe.cpu().numpy()) == bytes(fg.cpu().numpy())
    assert rt.sincnet_train_read(g)["step"] == 3
    rt.close()


# ------------------------------------------------------------------------------------------------ accuracy
@gpu
@pytest.mark.parametrize("B,S,segment", [(2, 2071, 32), (2, 4003, 32), (2, 2071, 0), (2, 4003, 64)])
def test_feats_and_gradients_within_4x_of_torch_f32(B, S, segment):
    """segment 32 is one 32-deep k-chunk per partial; 64 is two, and 0 (the default, 2048) puts a whole stage into one partial of up
    to 23 chunks: the chunk loop of the weight-gradient kernel and its bias partial across chunks."""
    cases = []
    for seed in SEEDS[(B, S)]:                                           # the float64 reference stays clear of every decision: CPU only
        p, wav_h, df_h = R.make_case(B, S, seed)
        m, dev, ok = R.decision_clearance(p, wav_h)
        print(f"seed {seed}: margins {[{k: float(f'{v:.3g}') for k, v in s.items()} for s in m]} f32 deviations { {k: float(f'{v:.3g}') for k, v in dev.items()} }")
        assert ok, (seed, m, dev)
        cases.append((p, wav_h, df_h))
    err = {}
    for p, wav_h, df_h in cases:
        ref_f, cache = R.forward(p, wav_h)
        ref_g, bias_abs = R.backward(p, cache, df_h)
        t32_f, t32_g, _ = R.torch_forward_backward(p, wav_h, df_h, torch.float32)
        rt = _model(p).runtime(_dev())
        t, f, g = _run(rt, _to(wav_h), _to(df_h), 0, segment)
        got = R.unpack(g)
        assert t.canaries_intact()
        rt.close()
        for k, ref, a, b in [("feats", ref_f, f.cpu().numpy(), t32_f)] + [(k, ref_g[k], got[k], t32_g[k]) for k, _ in R.keys()]:
            scale = bias_abs[k].max() if k in bias_abs else np.abs(ref).max()
            for who, v in (("kernel", a), ("torch", b)):
                d = (np.asarray(v, np.float64) - ref) / scale
                err.setdefault(k, {}).setdefault(who, []).append((float(np.abs(d).max()), float((d ** 2).mean())))
    bad = []
    for k, e in err.items():
        mx = {w: max(x[0] for x in e[w]) for w in e}
        rms = {w: float(np.sqrt(np.mean([x[1] for x in e[w]]))) for w in e}
        print(f"{k:32s} max kernel {mx['kernel']:.3e} torch {mx['torch']:.3e} ratio {mx['kernel'] / mx['torch']:.2f} | "
              f"rms kernel {rms['kernel']:.3e} torch {rms['torch']:.3e} ratio {rms['kernel'] / rms['torch']:.2f}")
        if not (mx["kernel"] <= 4.0 * mx["torch"] and rms["kernel"] <= 4.0 * rms["torch"]):
            bad.append(k)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ optimiser
@gpu
def test_apply_is_the_numpy_f32_adam_bit_for_bit():
    B, S = 2, 2071
    p, wav_h, df_h = R.make_case(B, S, 2)
    rt = _model(p).runtime(_dev())
    t = Trainer(rt, lr=3e-3)
    w = t.read(t.L.HEAD_TRAIN_MASTERS)
    assert np.array_equal(_bits(w), _bits(R.pack(p)))
    st = HR.adam_init(t.P)
    for k in range(3):
        _, wav_k, df_k = R.make_case(B, S, 60 + k)
        t.forward(_to(wav_k)), t.backward(_to(wav_k), _to(df_k))
        acc, frames = t.grad(), t.read(t.L.HEAD_TRAIN_SCALARS)["frames"]
        w, st = HR.adam_step(w, acc, frames, st, lr=3e-3)
        t.apply()
        assert np.array_equal(_bits(t.read(t.L.HEAD_TRAIN_MASTERS)), _bits(w)), k
        assert np.array_equal(_bits(t.read(t.L.HEAD_TRAIN_M)), _bits(st["m"])) and np.array_equal(_bits(t.read(t.L.HEAD_TRAIN_V)), _bits(st["v"]))
        assert not _bits(t.grad()).any() and t.read(t.L.HEAD_TRAIN_SCALARS)["t"] == k + 1
    assert t.canaries_intact()
    rt.close()


CHAIN_SEEDS = {183: 5, 2: 4, 30: 4}      # seed -> steps its float64 trajectory stays clear of every decision (searched on the CPU, seeds 0 .. 299)


@gpu
def test_full_steps_track_the_float64_torch_loop():
    """SincNet -> one 64-unit bidirectional LSTM layer -> a 32 / 1 head at (2, 2071), Adam on every tensor: the losses of the device's
    steps against the float64 torch loop, within 4 x the deviation of torch's own f32 loop.  Among seeds 0 .. 299 one (183) keeps the
    float64 trajectory clear of every decision for five steps (decision_clearance on the parameters each step starts from); seeds 2 and
    30 do for four, and run four.  The condition is asserted here on the CPU first."""
    dev2 = {"kernel": [], "torch": []}
    for seed, steps in CHAIN_SEEDS.items():
        p, rest, wav_h, y_h = R.chain_case(seed)
        l64, clear = R.chain_loop(p, rest, wav_h, y_h, steps, torch.float64, check=True)
        assert clear == steps, (seed, clear)
        l32, _ = R.chain_loop(p, rest, wav_h, y_h, steps, torch.float32)
        m = _model(p)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in rest.items()}, strict=False)
        rt = m.runtime(_dev())
        wav, y = _to(wav_h), _to(y_h)
        hh, hl, hs = rt.head_train_open(lr=1e-3, segment=32), rt.lstm_train_open(layers=1, lr=1e-3, segment=32), rt.sincnet_train_open(lr=1e-3, segment=32)
        got = []
        for _ in range(steps):
            f = rt.sincnet_train_forward(hs, wav)
            o = rt.lstm_train_forward(hl, f)
            _, gx = rt.head_train_grad(hh, o, y, want_grad_x=True)
            got.append(rt.head_train_batch_loss(hh).clone())
            gin = rt.lstm_train_backward(hl, f, gx, want_grad_in=True)
            rt.sincnet_train_backward(hs, wav, gin)
            rt.head_train_apply(hh), rt.lstm_train_apply(hl), rt.sincnet_train_apply(hs)
        torch.cuda.synchronize()
        got = np.array([float(l) for l in got])
        print(f"seed {seed}: float64 {l64[0]:.6f} -> {l64[-1]:.6f}, kernel {got[0]:.6f} -> {got[-1]:.6f}, "
              f"max deviation kernel {np.abs(got - l64).max():.3e} torch f32 {np.abs(l32 - l64).max():.3e}")
        dev2["kernel"] += list((got - l64) ** 2)
        dev2["torch"] += list((l32 - l64) ** 2)
        assert got[-1] < got[0] and rt.sincnet_train_read(hs)["step"] == steps
        rt.close()
    k, t = (float(np.sqrt(np.mean(dev2[w]))) for w in ("kernel", "torch"))
    print(f"rms deviation of the losses from the float64 loop: kernel {k:.3e}, torch f32 {t:.3e}, ratio {k / t:.2f}")
    assert k <= 4.0 * t


# ------------------------------------------------------------------------------------------------ commit and host layer
@gpu
def test_commit_serves_the_trained_front_end_and_leaves_other_contexts_alone():
    B, S = 2, 4003                                                       # 12 frames: the inference forms' documented bounds hold from 8 frames on
    p, wav_h, df_h = R.make_case(B, S, 1)
    model = _model(p)
    rt, other = model.runtime(_dev()), _model(p).runtime(_dev())
    wav, df = _to(wav_h), _to(df_h)
    before = other.sincnet(wav).clone()                                  # the default form
    assert other.sincnet_form() == "f16p"
    h = rt.sincnet_train_open(lr=1e-2, segment=32)
    for _ in range(2):
        rt.sincnet_train_forward(h, wav), rt.sincnet_train_backward(h, wav, df), rt.sincnet_train_apply(h)
    feats = rt.sincnet_train_forward(h, wav).clone()
    sd = rt.sincnet_train_state_dict(h)
    assert [k for k, _ in rt.sincnet_train_keys(0)] == ["sincnet." + k for k, _ in R.keys()] == list(sd)
    assert not torch.equal(sd["sincnet.conv1d.0.filterbank.low_hz_"], torch.from_numpy(p["conv1d.0.filterbank.low_hz_"]))
    rt.sincnet_train_commit(h)
    served16 = rt.sincnet(wav).clone()                                   # the default inference form serves the committed front end
    assert rt.sincnet_form() == "f16p"
    rt.set_gemm_mode("f32")                                              # the exact-f32 inference form
    served = rt.sincnet(wav)
    assert rt.sincnet_form() == "f32"
    # the exact-f32 inference form against the training forward: both f32 evaluations of the same network from the same weights and bank
    p_new = {k[len("sincnet."):]: v.numpy() for k, v in sd.items()}
    ref_f, _ = R.forward(p_new, wav_h)
    t32_f, _, _ = R.torch_forward_backward(p_new, wav_h, df_h, torch.float32)
    scale = np.abs(ref_f).max()
    e_train, e_inf, e_t32 = (float(np.abs(a - ref_f).max() / scale) for a in (feats.cpu().numpy(), served.cpu().numpy(), t32_f))
    print(f"feats error over max-abs: training forward {e_train:.3e}, served exact-f32 form {e_inf:.3e}, torch f32 {e_t32:.3e}")
    assert e_inf <= 4.0 * e_t32 and e_train <= 4.0 * e_t32
    # the default (split-f16) form: what tests/test_gpu_sincnet.py documents for it against the exact-f32 form -- no further from float64
    # than 1.5 x the exact-f32 form on rms, and both within 1e-4 at the worst value -- so it is within 2e-4 of the training forward
    rms = lambda a: float(np.sqrt(((a - ref_f) ** 2).mean()))
    r16, r32 = rms(served16.cpu().numpy()), rms(served.cpu().numpy())
    d16 = float(np.abs(served16.cpu().numpy() - feats.cpu().numpy()).max())
    print(f"served split-f16 form: rms {r16:.3e} against exact-f32 {r32:.3e}; max distance to the training forward {d16:.3e}")
    assert r16 <= 1.5 * r32 + 1e-9 and np.abs(served16.cpu().numpy() - ref_f).max() < 1e-4 and d16 <= 2e-4
    assert torch.equal(other.sincnet(wav), before) and not torch.equal(served16, before)   # another context with the same weights keeps them
    rt.close(), other.close()


@gpu
def test_vadmodel_train_step_trains_a_pyannet_and_commits_every_tensor():
    from uvad_amd.engine import VadModel
    md = {"lstm": {"hidden_size": 64, "num_layers": 1, "bidirectional": True, "dropout": 0.0}, "linear": {"hidden_size": 32, "num_layers": 1}}
    torch.manual_seed(5)
    vm = VadModel("PyanNet", md, learning_rate=1e-2).to(_dev()).eval()
    init = {k: v.detach().cpu().clone() for k, v in vm.state_dict().items()}
    B, S = 2, 2071
    T = R.num_frames(S)
    g = torch.Generator().manual_seed(6)
    batch = {"inputs": (0.1 * torch.randn(B, 1, S, generator=g)).to(_dev()), "is_voice": (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8)}
    losses = [vm.train_step(batch, k) for k in range(3)]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(l)) for l in losses)
    held = vm._adapt_full
    assert held[2]["layers"] == 1 and held[4]["first_stage"] == 0 and held[0].sincnet_train_read(held[4])["step"] == 3
    vm.train_commit()
    sd = vm.state_dict()
    for k in ("model.sincnet.conv1d.0.filterbank.low_hz_", "model.sincnet.conv1d.1.weight", "model.sincnet.norm1d.2.bias", "model.classifier.weight"):
        assert not torch.equal(sd[k].cpu(), init[k]), k
    probs = vm.model(batch["inputs"])
    assert tuple(probs.shape) == (B, T, 1) and bool(torch.isfinite(probs).all())
    vm.adapt_step({"inputs": batch["inputs"][:, 0], "is_voice": batch["is_voice"]}, 0, sincnet_stages=1)      # (B, S); the top stage only
    assert vm._adapt_full[4]["first_stage"] == 2 and vm._adapt_full[4]["P"] == 18180
    with pytest.raises(NotImplementedError, match="SincNet"):
        vm.train_step(dict(batch, lengths=[T, T]), 0)
    with pytest.raises(NotImplementedError, match="SincNet"):
        vm.adapt_step(dict(batch, lengths=[T, T]), 0, sincnet_stages=2)
    with pytest.raises(NotImplementedError):
        vm.training_step({}, 0)
    with pytest.raises(NotImplementedError):
        vm.configure_optimizers()


@gpu
def test_train_vad_trains_a_pyannet_on_waveform_windows_and_writes_its_checkpoint(tmp_path, capfd):
    import wave
    import main as entry
    from config.config import load_config
    from uvad_amd.engine import VadModel
    from uvad_amd.synth import synth_pcm
    paths, labels = [], []
    for k in range(2):
        x = synth_pcm(1, int(1.2 * 16000) + 300 * (1 - k), seed=700 + k)[0]      # 1.2 s; the first file's tail is 300 samples: no frame
        x[int(0.3 * 16000):int(0.6 * 16000)] *= 0.02
        p, f = tmp_path / f"a{k}.wav", tmp_path / f"a{k}.txt"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
        f.write_text("0.0\t0.3\tSPC\n0.6\t1.2\tSPC\n")
        paths.append(str(p)); labels.append(str(f))
    cfg = load_config()
    cfg.feature_extractor, cfg.model_name = "sincnet", "PyanNet"
    cfg.model_dict.encoding_dim = 60
    cfg.model_dict.lstm = {"hidden_size": 64, "num_layers": 1, "dropout": 0.0}
    cfg.model_dict.linear = {"hidden_size": 32, "num_layers": 1}
    cfg.input.kind, cfg.input.paths, cfg.input.labels = "wav", paths, labels
    cfg.function, cfg.learning_rate, cfg.max_epochs, cfg.check_val_every_n_epoch = "train", 1e-2, 2, 2
    cfg.window_seconds, cfg.max_duration, cfg.accumulate_grad_batches = 0.4, 0.8, 1
    cfg.experiments_dir = str(tmp_path / "wave")
    got = entry.main(cfg)                                                        # function = "train" reaches train_vad
    # 3 full windows of 6400 samples per file, two rows per batch: 3 batches per epoch; the second file's tail is empty, the first one's skipped
    assert "1 tail window(s) shorter than the receptive field" in capfd.readouterr().out
    assert got["global_step"] == 3 * 2 and [e for e, _ in got["val_loss"]] == [2]
    assert len(got["train_loss"]) == 2 and np.isfinite(got["train_loss"]).all() and np.isfinite([l for _, l in got["val_loss"]]).all()
    assert got["checkpoint_path"] == str(tmp_path / "wave" / "checkpoint-epoch=02.ckpt")
    blob = torch.load(got["checkpoint_path"], weights_only=True)
    torch.manual_seed(cfg.seed)
    init = VadModel("PyanNet", dict(cfg.model_dict)).state_dict()                # torch's own initialisation under the run's seed
    assert set(blob["state_dict"]) == set(init)
    moved = [k for k in init if k.startswith("model.sincnet.") and not k.endswith(("window_", "n_"))]
    assert len(moved) == 14
    for k in moved:                                                              # every sincnet.* tensor differs from its initial value
        assert not torch.equal(blob["state_dict"][k], init[k]), k
