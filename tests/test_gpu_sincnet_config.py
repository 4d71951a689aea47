"""GPU parity tests (-m gpu) of the SincNet front end OFF the reference point: every geometry, leaky slope and eps that
uvad_sincnet_configure accepts is reachable through VadRuntime(device, model=..., sincnet=cfg), and each case is held to the
standard of test_gpu_sincnet.py::test_sincnet_split_f16_stages_against_the_exact_f32_stages_and_the_float64_truth:

  * against the float64 evaluation of the same network (oracle/parity_stats.py: truth_sincnet, parametric): max-abs < 1e-4 for
    outputs of >= 8 frames, 5e-4 for shorter ones (the instance norm of a few values divides by ~sqrt(eps)), times max(1, |slope|)
    where the slope multiplies the output;
  * the split-f16 form (sincnet_f16p.hip) no further from that truth than 1.5 x the exact-f32 form (sincnet.hip) on rms;
  * the form that ran (uvad_get_sincnet_form) asserted on every call, so that no silent fall-back can leave the f16 kernels untested.

Configurations the library refuses are asserted as refusals (code and message), not skipped.  The classifier's leaky_slope is held
to the C oracle (oracle/uvad_oracle.c) through every kernel that applies it."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FEAT_TOL = 1e-4
SHORT_TOL = 5e-4
LOGIT_TOL = 1e-4
REL = 1.5
TILE16 = 64                   # pooled outputs per tile of the split-f16 stages
LDS = 160 * 1024
MODES = ("f16p", "f16p3", "f32")
SMALL_CLS = dict(hidden=64, num_layers=1, bidirectional=False, lin_hidden=128, lin_layers=0)   # the sweep's classifier: cheap to pack

REF = dict(stride=10, n_filters=80, kernel_size=251, c2=60, k2=5, c3=60, k3=5)


def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


# ---------------------------------------------------------------------------------------------------------------------------------
# What the library does with a configuration, restated from uvad_sincnet_configure / sinc_conv_plan (sincnet.hip) and
# sinc_f16p_supported (sincnet_f16p.hip): which ones it refuses and why, the exact form's tile (pooled outputs per workgroup tile) of
# every stage, and whether modes f16p / f16p3 run the split-f16 stages.

def _stages(cfg):
    return ((1, cfg["kernel_size"], cfg["stride"], cfg["n_filters"]), (cfg["n_filters"], cfg["k2"], 1, cfg["c2"]),
            (cfg["c2"], cfg["k3"], 1, cfg["c3"]))


def _lds_ept(cin, kw, stride, cout, waves):
    nw = (cout + 31) // 32 * 32
    kp = (cin * kw + 7) // 8 * 8
    xw = (waves * 32 - 1) * stride + kw
    lds = (kp * nw + max(cin * xw + 9, nw * 97)) * 4 + 96 * 8
    return lds, (cin * xw + waves * 64 - 1) // (waves * 64)


def _exact_tiles(cfg):
    pts = []
    for cin, kw, stride, cout in _stages(cfg):
        if cin == 1:
            lds, ept = _lds_ept(cin, kw, stride, cout, 8)
            waves = 8 if lds <= LDS and ept <= 8 else 3
        else:
            lds, ept = _lds_ept(cin, kw, stride, cout, 4)
            waves = 4 if lds <= LDS and ept <= 48 else 3
        pts.append(waves * 32 // 3)
    return pts


def _refusal(cfg):
    """None if uvad_sincnet_configure accepts cfg (with encoding_dim = c3), else the words of its message."""
    if cfg["n_filters"] % 2 or cfg["c2"] % 2:
        return "must be even"
    if any(not 32 < c <= 96 for c in (cfg["n_filters"], cfg["c2"], cfg["c3"])):
        return "must be in 33..96"
    for cin, kw, stride, cout in _stages(cfg):
        lds, ept = _lds_ept(cin, kw, stride, cout, 3)
        if lds > LDS:
            return "does not fit the 160 KiB LDS"
        if ept > (8 if cin == 1 else 48):
            return "input window too large"
    return None


def _f16_geometry(cfg):
    return (cfg["stride"] == 10 and cfg["kernel_size"] <= 256 and cfg["n_filters"] == 80 and cfg["k2"] == 5 and cfg["c2"] <= 64
            and cfg["c2"] % 4 == 0 and cfg["k3"] == 5 and cfg["c3"] <= 64)


def _length(front, stage, pooled, slack):
    """The shortest waveform whose stage `stage` has exactly `pooled` pooled outputs, plus `slack` < 3 x stride samples (which changes
    no stage's count)."""
    n = pooled
    for kw, st in ((front.kernel_size, front.stride), (front.k2, 1), (front.k3, 1))[stage::-1]:
        n = (3 * n - 1) * st + kw
    return n + slack


def _edge_lengths(front, tiles, phase, rng):
    """One length per stage: that stage ends one before, on, or one after a tile edge (offset rotated by `phase` and the stage), at the
    smallest multiple of the tile that leaves >= 8 output frames."""
    out = []
    for stage, t in enumerate(tiles):
        off = (stage + phase) % 3 - 1
        k = 1
        while True:
            S = _length(front, stage, k * t + off, int(rng.integers(0, 3 * front.stride)))
            if front.num_frames(S) >= 8 or S > 60000:
                break
            k += 1
        assert front.num_frames(S) >= 1 and S <= 80000, (front.config(), stage, t, S)
        out.append(S)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------

def _model(c3, slope=0.01, hidden=128, num_layers=4, bidirectional=True, lin_hidden=128, lin_layers=2):
    return {"encoding_dim": c3, "lstm": {"hidden_size": hidden, "num_layers": num_layers, "bidirectional": bidirectional},
            "linear": {"hidden_size": lin_hidden, "num_layers": lin_layers}, "leaky_slope": slope}


def _mcfg(model):
    from oracle import c_oracle as co
    l, n = model["lstm"], model["linear"]
    return co.ModelCfg(model["encoding_dim"], l["hidden_size"], l["num_layers"], int(l["bidirectional"]), n["hidden_size"],
                       n["num_layers"], model["leaky_slope"])


def _runtime(front, cls=SMALL_CLS, model_slope=0.01, seed=4321, scale=2.0):
    """(VadRuntime with `front`'s configuration and tensors plus seeded classifier weights, model dict, classifier state dict)."""
    import uvad_amd
    from oracle import torch_ref as tr
    model = _model(front.c3, model_slope, **cls)
    csd = tr.seeded_state_dict(front.c3, cls["hidden"], cls["num_layers"], cls["bidirectional"], cls["lin_hidden"], cls["lin_layers"],
                               seed=seed, scale=scale)
    rt = uvad_amd.VadRuntime(torch.device("cuda:0"), model=model, sincnet=front.config())
    rt.load_state_dict(tr.sincnet_runtime_state_dict(front, csd))
    return rt, model, csd


def _run(rt, wav, mode):
    rt.set_gemm_mode(mode)
    out = rt.sincnet(wav.cuda()).cpu()
    return out, rt.sincnet_form()


def _check(rt, front, wav, f16, label, rel=False):
    """Every mode against the float64 truth; the forms asserted; the split-f16 form's rms against the exact form's.  Returns the
    outputs by mode."""
    from oracle import parity_stats as ps
    truth = ps.truth_sincnet(front, wav).numpy()
    got, forms, errs = {}, {}, {}
    for mode in MODES:
        g, forms[mode] = _run(rt, wav, mode)
        got[mode] = g
        errs[mode] = np.abs(g.numpy().astype(np.float64) - truth)
    rt.set_gemm_mode("f16p")
    frames = truth.shape[1]
    act = max(1.0, abs(front.leaky_slope))
    tol = (FEAT_TOL if frames >= 8 else SHORT_TOL) * act
    if rel:   # outputs scaled by a huge slope: the error is measured against the output's own scale
        tol = FEAT_TOL * max(1.0, float(np.abs(truth).max()))
    rms = {m: float(np.sqrt((e ** 2).mean())) for m, e in errs.items()}
    line = (f"{label} B={wav.shape[0]} S={wav.shape[1]} frames {frames}: " +
            "; ".join(f"{m}[{forms[m]}] max {errs[m].max():.2e} rms {rms[m]:.2e}" for m in MODES))
    print(line)
    for m in MODES:
        assert got[m].shape == truth.shape == (wav.shape[0], front.num_frames(wav.shape[1]), front.c3)
        assert errs[m].max() < tol, (label, m, forms[m], float(errs[m].max()), tol)
    want = {"f16p": "f16p" if f16 else "f32", "f16p3": "f16p" if f16 else "f32", "f32": "f32"}
    assert forms == want, (label, forms, want)
    assert torch.equal(got["f16p"], got["f16p3"])          # modes 1 and 3 run the same SincNet stages
    if f16:
        assert rms["f16p"] <= REL * rms["f32"] + 1e-9, (label, rms)
    else:
        assert torch.equal(got["f16p"], got["f32"])        # one form in every mode
    return got


def _check_i16(rt, front, B, S, f16, seed):
    """int16 ingest: the _i16 call equals the f32 call on q.float() / 32768 bit for bit, in both forms."""
    from oracle import torch_ref as tr
    q = torch.from_numpy(np.round(tr.synth_pcm(B, S, seed=seed) * 32767.0).astype(np.int16))
    for mode in (("f16p", "f32") if f16 else ("f32",)):
        rt.set_gemm_mode(mode)
        a = rt.sincnet(q.cuda()).cpu()
        fa = rt.sincnet_form()
        b = rt.sincnet((q.float() / 32768).cuda()).cpu()
        assert fa == rt.sincnet_form() == ("f16p" if mode == "f16p" and f16 else "f32")
        assert torch.equal(a, b), (front.config(), mode, float((a - b).abs().max()))
    rt.set_gemm_mode("f16p")


def _assert_refused(cfg, words):
    import uvad_amd
    from uvad_amd._lib import UvadError
    with pytest.raises(UvadError) as ei:
        uvad_amd.VadRuntime(torch.device("cuda:0"), model=_model(cfg["c3"], **SMALL_CLS), sincnet=dict(cfg, leaky_slope=0.01, eps=1e-5))
    assert ei.value.code == -5 and "UVAD_E_UNSUPPORTED" in str(ei.value) and words in str(ei.value), (cfg, str(ei.value))


def _sweep(cfgs, seed):
    from oracle import torch_ref as tr
    _threads()
    rng = np.random.default_rng(seed)
    ran = refused = 0
    for idx, cfg in enumerate(cfgs):
        full = dict(REF, **cfg)
        full.setdefault("leaky_slope", 0.01)
        full.setdefault("eps", 1e-5)
        geo = {k: full[k] for k in REF}
        words = _refusal(geo)
        if words is not None:
            _assert_refused(geo, words)
            print(f"{geo}: refused ({words})")
            refused += 1
            continue
        front = tr.seeded_sincnet(int(rng.integers(0, 1 << 30)), **full)
        rt, _, _ = _runtime(front)
        f16 = _f16_geometry(geo) and full["leaky_slope"] <= 1.0
        tiles = [_exact_tiles(geo)] + ([[TILE16] * 3] if _f16_geometry(geo) else [])
        lengths = [S for t in tiles for S in _edge_lengths(front, t, idx, rng)]
        for j, S in enumerate(lengths):
            B = int(rng.integers(1, 6))
            wav = torch.from_numpy(tr.synth_pcm(B, S, seed=int(rng.integers(0, 10000))))
            _check(rt, front, wav, f16, str(cfg))
            if idx % 3 == 0 and j == 0:
                _check_i16(rt, front, B, S, f16, seed=int(rng.integers(0, 10000)))
        rt.close()
        ran += 1
    return ran, refused


def test_sincnet_geometry_sweep_inside_the_split_f16_subspace():
    """Named points of the split-f16 subspace (stride 10, 80 filters, <= 256 taps, k2 = k3 = 5, c2 <= 64 with c2 % 4 == 0, c3 <= 64):
    shorter filter banks (zero-weight taps) and zero-padded channel tiles (c2 < 64, c3 < 60).  Modes f16p / f16p3 must run "f16p",
    mode f32 "f32"; lengths put every stage on, one before and one after a tile edge of both forms."""
    cfgs = [dict(kernel_size=k) for k in (3, 129, 250, 256)] + [dict(c2=c) for c in (36, 48, 64)] + [dict(c3=c) for c in (36, 40, 44, 64)]
    for c in cfgs:
        assert _f16_geometry(dict(REF, **c)) and _refusal(dict(REF, **c)) is None, c
    ran, refused = _sweep(cfgs, 11)
    assert ran == len(cfgs) and refused == 0


def test_sincnet_geometry_sweep_outside_the_split_f16_subspace():
    """Points outside the split-f16 subspace run the exact-f32 stages in every mode; the ones uvad_sincnet_configure refuses (the LDS-resident
    filter matrix, the register-staged input window) are asserted as UVAD_E_UNSUPPORTED with their message.  k2 = 6 at 80 -> 60 channels
    takes the 3-wave workgroup (32 pooled outputs per tile) of the multi-channel stages; Conv1d(78 -> 46, 6) needs 163 132 of the 163 840
    bytes of LDS in its 4-wave form (its launch failed while the static (scale, shift) table was requested a second time as dynamic LDS)."""
    cfgs = ([dict(stride=s) for s in (1, 3)] + [dict(stride=16, kernel_size=15), dict(stride=16)] +
            [dict(n_filters=n) for n in (34, 64, 96)] + [dict(c2=c) for c in (34, 66, 96)] + [dict(c3=c) for c in (68, 96)] +
            [dict(k2=k) for k in (3, 4, 6, 7, 9)] + [dict(k3=k) for k in (3, 4, 7, 9)] + [dict(kernel_size=301), dict(kernel_size=512)] +
            [dict(n_filters=48, k2=7), dict(c2=40, k3=9), dict(n_filters=78, c2=46, k2=6)])
    for c in cfgs:
        assert not _f16_geometry(dict(REF, **c)), c
    ran, refused = _sweep(cfgs, 12)
    print(f"outside the split-f16 subspace: {ran} configurations run, {refused} refused")
    assert ran >= 16 and refused >= 4


def test_sincnet_geometry_sweep_random_draw():
    """A seeded draw of accepted configurations (about half inside the split-f16 subspace), with random slopes and eps; refused draws are
    asserted as refusals on the way."""
    rng = np.random.default_rng(2024)
    cfgs = []
    accepted = 0
    while accepted < 10:
        if rng.random() < 0.45:
            c = dict(stride=10, n_filters=80, kernel_size=int(rng.integers(3, 257)), c2=int(rng.integers(9, 17)) * 4, k2=5,
                     c3=int(rng.integers(9, 17)) * 4, k3=5)
        else:
            c = dict(stride=int(rng.integers(1, 17)), n_filters=int(rng.integers(17, 49)) * 2, kernel_size=int(rng.integers(3, 330)),
                     c2=int(rng.integers(17, 49)) * 2, k2=int(rng.integers(3, 10)), c3=int(rng.integers(9, 25)) * 4, k3=int(rng.integers(3, 10)))
        c["leaky_slope"] = float(rng.choice([0.01, -0.3, 0.0, 0.7, 1.0, 2.0]))
        c["eps"] = float(rng.choice([1e-5, 1e-3, 0.1]))
        cfgs.append(c)
        accepted += _refusal({k: c[k] for k in REF}) is None
    ran, refused = _sweep(cfgs, 13)
    print(f"random draw: {ran} configurations run, {refused} refused")
    assert ran == 10


@pytest.mark.parametrize("geo", [dict(c3=36), dict(c3=96), dict(kernel_size=129, c2=48), dict(stride=3, n_filters=64, k3=4)])
def test_pyannet_forward_wav_off_the_reference_geometry(geo):
    """The whole model at other geometries (encoding_dim = c3): forward_wav's logits are classify(sincnet(wav)) on the same context bit
    for bit (the same kernels on the same features in the same workspace order), and within LOGIT_TOL of the C oracle's classifier on the
    float64 features, with weights at scale 1 and 2."""
    from oracle import c_oracle as co, parity_stats as ps, torch_ref as tr
    _threads()
    cfg = dict(REF, **geo)
    f16 = _f16_geometry(cfg)
    front = tr.seeded_sincnet(31, **cfg)
    wav = torch.from_numpy(tr.synth_pcm(3, 24011, seed=41))
    f64 = ps.truth_sincnet(front, wav).numpy()
    for scale in (1.0, 2.0):
        rt, model, csd = _runtime(front, cls=dict(hidden=128, num_layers=2, bidirectional=True, lin_hidden=128, lin_layers=2), scale=scale)
        want, _ = co.classify({k: v.numpy() for k, v in csd.items()}, _mcfg(model), f64.astype(np.float32))
        for mode in MODES:
            rt.set_gemm_mode(mode)
            logits, probs = rt.forward_wav(wav.cuda())
            form = rt.sincnet_form()
            feats = rt.sincnet(wav.cuda())
            assert rt.sincnet_form() == form == ("f16p" if f16 and mode != "f32" else "f32")
            lg2, pr2 = rt.classify(feats)
            assert torch.equal(logits, lg2) and torch.equal(probs, pr2), (geo, mode, float((logits - lg2).abs().max()))
            err = float(np.abs(logits.cpu().numpy() - want).max())
            print(f"{geo} x{scale:g} {mode}[{form}]: logits {tuple(logits.shape)} vs C oracle on the float64 features {err:.2e}")
            assert logits.shape == want.shape and err < LOGIT_TOL, (geo, scale, mode, err)
        rt.close()


# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slope", [-3.0, -0.2, 0.0, 0.5, 1.0, 1.5, 4.0])
def test_sincnet_leaky_slope_at_the_reference_geometry(slope):
    """Any slope <= 1 (negative ones included) is leaky_relu in the split-f16 staging (max(e, e * slope)); a slope > 1 is not, so the
    library runs the exact-f32 stages for it in every mode.  Parity with the float64 truth either way."""
    from oracle import torch_ref as tr
    _threads()
    front = tr.seeded_sincnet(77, leaky_slope=slope)
    rt, _, _ = _runtime(front)
    for B, S in ((3, 24011), (1, 80000)):
        wav = torch.from_numpy(tr.synth_pcm(B, S, seed=int(S % 997)))
        _check(rt, front, wav, slope <= 1.0, f"slope {slope:g}")
    rt.close()


def test_sincnet_huge_slope_leaves_the_f16_range_and_runs_the_exact_stages():
    """slope -2e4: the stage inputs after leaky_relu exceed what the split-f16 staging may convert ((|gamma| sqrt(L) + |beta|) x |slope| >=
    60000), so every mode runs the exact-f32 stages; parity on the error relative to the output's scale."""
    from oracle import torch_ref as tr
    _threads()
    front = tr.seeded_sincnet(78, leaky_slope=-2e4)
    rt, _, _ = _runtime(front)
    wav = torch.from_numpy(tr.synth_pcm(2, 24011, seed=5))
    _check(rt, front, wav, False, "slope -2e4", rel=True)
    rt.close()


@pytest.mark.parametrize("eps", [1e-3, 1.0])
def test_sincnet_eps_at_the_reference_geometry(eps):
    from oracle import torch_ref as tr
    _threads()
    front = tr.seeded_sincnet(79, eps=eps)
    rt, _, _ = _runtime(front)
    for B, S in ((2, 24011), (4, 4000)):
        _check(rt, front, torch.from_numpy(tr.synth_pcm(B, S, seed=S % 991)), True, f"eps {eps:g}")
    rt.close()


def test_non_finite_slope_or_eps_and_negative_eps_are_refused():
    import uvad_amd
    from uvad_amd._lib import UvadError
    dev = torch.device("cuda:0")
    bad = [("leaky_slope", float("nan")), ("leaky_slope", float("inf")), ("leaky_slope", -float("inf")),
           ("eps", float("nan")), ("eps", float("inf")), ("eps", -1e-6)]
    for key, v in bad:
        with pytest.raises(UvadError) as ei:
            uvad_amd.VadRuntime(dev, model=_model(60, **SMALL_CLS), sincnet=dict(REF, **{"leaky_slope": 0.01, "eps": 1e-5, key: v}))
        assert ei.value.code == -1 and "UVAD_E_ARG" in str(ei.value) and key in str(ei.value), (key, v, str(ei.value))
    for v in (float("nan"), float("inf")):
        with pytest.raises(UvadError) as ei:
            uvad_amd.VadRuntime(dev, model=_model(60, v, **SMALL_CLS))
        assert ei.value.code == -1 and "UVAD_E_ARG" in str(ei.value) and "leaky_slope" in str(ei.value), str(ei.value)
    # the boundaries stay accepted
    uvad_amd.VadRuntime(dev, model=_model(60, -1e30, **SMALL_CLS), sincnet=dict(REF, leaky_slope=-1e30, eps=0.0)).close()


# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slope", [-0.5, 0.0, 1.0, 2.5])
def test_classifier_leaky_slope_through_every_kernel_that_applies_it(slope):
    """uvad_model_cfg.leaky_slope against the C oracle with the same slope: the exact-f32 head GEMM (mode f32), the split-f16 one (f16p_stream,
    and a 1-layer head in f16p), the fused head (f16p / f16p3 with the default 2 x 128 head), the 16-sequence recurrent tile, and the
    streaming step's in-launch head (lstm_stack.hip) of a causal model against the offline path and the oracle."""
    import uvad_amd
    from uvad_amd.synth import synth_pcm
    from oracle import c_oracle as co, torch_ref as tr
    dev = torch.device("cuda:0")
    x = torch.randn(5, 150, 64, generator=torch.Generator().manual_seed(3)) * 2 - 1
    for lin_layers, modes in ((2, ("f32", "f16p_stream", "f16p", "f16p3")), (1, ("f32", "f16p"))):
        model = _model(64, slope, 128, 2, True, 128, lin_layers)
        sd = tr.seeded_state_dict(64, 128, 2, True, 128, lin_layers, seed=17, scale=2.0)
        want, _ = co.classify({k: v.numpy() for k, v in sd.items()}, _mcfg(model), x.numpy())
        rt = uvad_amd.VadRuntime(dev, model=model)
        rt.load_state_dict(sd)
        for mode in modes:
            rt.set_gemm_mode(mode)
            for tile in ((0, 16) if lin_layers == 2 and mode == "f16p" else (0,)):
                rt.set_recurrent_tile(tile)
                got = rt.classify(x.to(dev), want_probs=False)[0].cpu().numpy()
                assert tile == 0 or rt.recurrent_tile() == 16
                err = float(np.abs(got - want).max())
                print(f"classifier slope {slope:g}, {lin_layers}-layer head, {mode}, tile {rt.recurrent_tile()}: {err:.2e} "
                      f"(logits {want.min():.2f}..{want.max():.2f})")
                assert err < LOGIT_TOL, (slope, lin_layers, mode, tile, err)
            rt.set_recurrent_tile(0)
        rt.close()
    # the streaming step of a causal model with the 2 x 128 head
    B, S, F, chunk = 4, 16000, 64, 320
    model = _model(F, slope, 128, 2, False, 128, 2)
    sd = tr.seeded_state_dict(F, 128, 2, False, 128, 2, seed=18, scale=2.0)
    rt = uvad_amd.VadRuntime(dev, fbank=uvad_amd.FbankConfig(num_filters=F, window_type="povey"), model=model)
    rt.load_state_dict(sd)
    pcm = torch.from_numpy(synth_pcm(B, S, seed=19)).to(dev)
    offline, _ = rt.forward(pcm)
    st = rt.stream_open(B, chunk)
    got = torch.cat([rt.stream_step(st, pcm[:, i * chunk:(i + 1) * chunk].contiguous()).clone() for i in range(S // chunk)], dim=1)
    n = got.shape[1]
    assert n >= S // 160 - 2
    sdiff = float((got - offline[:, :n]).abs().max())
    feats = rt.fbank(pcm)
    want, _ = co.classify({k: v.numpy() for k, v in sd.items()}, _mcfg(model), feats.cpu().numpy())
    oerr = float(np.abs(offline.cpu().numpy() - want).max())
    print(f"classifier slope {slope:g}, causal stream of {chunk} samples: |stream - offline| {sdiff:.2e}, offline vs C oracle {oerr:.2e}")
    assert sdiff < LOGIT_TOL and oerr < LOGIT_TOL
    rt.close()


def test_weight_cache_is_keyed_by_slopes_and_eps():
    """Contexts with identical tensors that differ only in the SincNet slope, the SincNet eps or the model slope must not share packed weights
    (uvad_weights_shared_by() == 1 each) and each must match its own oracle; two with identical configuration share (2) and agree bit for bit."""
    from oracle import c_oracle as co, parity_stats as ps, torch_ref as tr
    _threads()
    dev = torch.device("cuda:0")
    variants = [dict(), dict(leaky_slope=0.3), dict(eps=1e-2), dict(model_slope=-0.4)]
    wav = torch.from_numpy(tr.synth_pcm(2, 16011, seed=23))
    rts, outs = [], []
    cls = dict(hidden=128, num_layers=1, bidirectional=True, lin_hidden=128, lin_layers=2)
    for v in variants:
        front = tr.seeded_sincnet(55, **{k: x for k, x in v.items() if k != "model_slope"})
        rt, model, csd = _runtime(front, cls=cls, model_slope=v.get("model_slope", 0.01), seed=8)
        rts.append(rt)
        feats = rt.sincnet(wav.to(dev))
        logits = rt.classify(feats, want_probs=False)[0]
        truth = ps.truth_sincnet(front, wav).numpy()
        ferr = float(np.abs(feats.cpu().numpy() - truth).max())
        want, _ = co.classify({k: x.numpy() for k, x in csd.items()}, _mcfg(model), feats.cpu().numpy())
        lerr = float(np.abs(logits.cpu().numpy() - want).max())
        print(f"{v or 'reference'}: features vs float64 {ferr:.2e}, logits vs C oracle {lerr:.2e}")
        assert rt.sincnet_form() == "f16p" and ferr < FEAT_TOL and lerr < LOGIT_TOL, (v, ferr, lerr)
        outs.append((feats.cpu(), logits.cpu()))
    assert [r.weights_shared_by() for r in rts] == [1, 1, 1, 1]
    for i in range(1, 4):
        assert not torch.equal(outs[i][0], outs[0][0]) or not torch.equal(outs[i][1], outs[0][1]), variants[i]
    twin, _, _ = _runtime(tr.seeded_sincnet(55), cls=cls, seed=8)
    assert twin.weights_shared_by() == 2 and rts[0].weights_shared_by() == 2 and [r.weights_shared_by() for r in rts[1:]] == [1, 1, 1]
    feats = twin.sincnet(wav.to(dev))
    assert torch.equal(feats.cpu(), outs[0][0]) and torch.equal(twin.classify(feats, want_probs=False)[0].cpu(), outs[0][1])
    for r in rts + [twin]:
        r.close()
