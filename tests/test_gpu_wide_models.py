"""GPU tests (-m gpu) of the models at the edges of what uvad_create accepts: hidden sizes above 256 (lstm_rec_any_kernel gives a thread the
units tid, tid + 256, tid + 512, tid + 768, so a second pass exists only there), up to the bound of 1024, down to hidden x directions = 32,
and feed-forward widths that are no multiple of 32 (the plane-writing epilogues of gemm_f16p_kernel then own the zero columns
[lin_hidden, round_up(lin_hidden, 32)) the next layer's K runs over).

  reference  the float64 evaluation of the same network on the same f32 weights and features (oracle.parity_stats.truth_logits; the taps
             from oracle.torch_ref.TorchPyanNet2(...).double())
  bound      LOGIT_TOL = 1e-4, the project's contract (tests/test_gpu_parity.py), on logits, probabilities, the LSTM tap and the
             feed-forward tap.  Weights x4: the logits span several units, the sequences (T <= 30) are too short for the chaotic tail of
             DESIGN section 4, and the fp32 torch CPU path sits at 2e-7 ... 9e-6 (logits), <= 3.3e-6 (LSTM tap), <= 8e-6 (feed-forward tap)
             from float64 on exactly these draws, ten times inside the bound; 16 zeroed units of the last layer move the logits by 0.09 ... 2.8
  workspace  every checked call runs on a workspace filled with 0xFF bytes (NaN in f32 and f16) after a call of the same shape has made it
             exist: a column, row or counter the call needs and does not write cannot hold the previous call's right answer
  bit for bit  batch placement (lane 0 and lane 3 of a full tile, lane 0 of a partial last one), run to run, a ragged batch against the
             dense call of each length alone (modes f32, f16p_stream), NaN / 1e30 in the padding frames

The ratio of the GPU's error to the fp32 CPU path's (rms over the LSTM tap) is printed, not asserted: the generic recurrence sums K up to
1024 as one k-ordered fmaf chain, the CPU in blocks.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
DEV = "cuda:0"
MODES = ("f32", "f16p", "f16p_stream", "f16p3")

# (F, hidden, layers, bidirectional, lin_hidden, lin_layers, B, T)
CASES = {
    "h272-bi-lin128x2": (64, 272, 2, True, 128, 2, 5, 12),     # second pass with 16 of 256 threads; layer-1 K = 544; 17 column tiles
    "h288-uni-lin100x3": (64, 288, 2, False, 100, 3, 6, 9),    # one direction; Zw = 128: whole-tile plane epilogue with N = 100 < ldc, twice
    "h512-bi-lin36x2": (80, 512, 2, True, 36, 2, 5, 10),       # two full passes; K = 1024; Zw = 64: masked plane epilogue with N = 36
    "h784-bi-lin260x2": (64, 784, 1, True, 260, 2, 3, 7),      # four passes, the last with 16 units; 49 column tiles; Zw = 288 (3 column tiles, masked)
    "h1024-bi-lin128x2": (64, 1024, 2, True, 128, 2, 5, 8),    # the upper bound: four full passes; K = 2048; N = 8192; head on 2048-wide planes
    "h1024-uni-lin0": (40, 1024, 1, False, 128, 0, 2, 5),      # no feed-forward: classifier_kernel at K = 1024 on f32 rows; F = 40 padded to 64
    "h16-bi-lin20x2": (64, 16, 2, True, 20, 2, 7, 30),         # the lower bound (H x D = 32, one column tile, 240 idle threads); Zw = 32
}
STRUCTURE_CASES = ("h272-bi-lin128x2", "h512-bi-lin36x2", "h784-bi-lin260x2")


@functools.lru_cache(maxsize=None)
def state_dict(name):
    from oracle import torch_ref as tr
    F, H, L, bi, lh, ll, _, _ = CASES[name]
    return tr.seeded_state_dict(F, H, L, bi, lh, ll, seed=77, scale=4.0)


def features(name, B=None):
    F, _, _, _, _, _, B0, T = CASES[name]
    g = torch.Generator().manual_seed(5)
    return torch.randn(B or B0, T, F, generator=g) * 2.0 - 3.0


def torch_model(name, double):
    from oracle import torch_ref as tr
    F, H, L, bi, lh, ll, _, _ = CASES[name]
    m = tr.TorchPyanNet2(F, H, L, bi, lh, ll)
    m.load_state_dict(state_dict(name))
    return m.double() if double else m


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 truth, the fp32 CPU path) of the case's batch, each {logits, probs, lstm, lin (None without feed-forward layers)} as float64
    numpy; computed once per process and never modified."""
    from oracle import parity_stats as ps
    F, H, L, bi, lh, ll, _, _ = CASES[name]
    x = features(name)
    out = []
    for double in (True, False):
        lg, pr, y, z = torch_model(name, double)(x.double() if double else x, taps=True)
        out.append({"logits": lg.double().numpy(), "probs": pr.double().numpy(), "lstm": y.double().numpy(),
                    "lin": z.double().numpy() if ll > 0 else None})
    truth = ps.truth_logits(state_dict(name), x, F, H, L, bi, lh, ll)
    assert np.abs(truth - out[0]["logits"]).max() < 1e-12   # the two float64 evaluations are the same operators on the same numbers
    out[0]["logits"] = truth
    for d in out:
        for v in d.values():
            if v is not None:
                v.setflags(write=False)
    return out[0], out[1]


_RUNTIMES = {}


def runtime(name):
    import uvad_amd
    rt = _RUNTIMES.get(name)
    if rt is None:
        F, H, L, bi, lh, ll, _, _ = CASES[name]
        model = {"encoding_dim": F, "lstm": {"hidden_size": H, "num_layers": L, "bidirectional": bi},
                 "linear": {"hidden_size": lh, "num_layers": ll}}
        rt = uvad_amd.VadRuntime(DEV, fbank=None, model=model)
        rt.load_state_dict(state_dict(name))
        _RUNTIMES[name] = rt
    return rt


def poisoned_classify(rt, feats, lengths=None):
    """rt.classify on a workspace whose every byte is 0xFF: one call of the same shape first, so that the workspace exists."""
    rt.classify(feats, lengths=lengths)
    rt._ws.fill_(0xFF)
    return rt.classify(feats, lengths=lengths)


def passes_of(H, D):
    """[(label, column slice of the LSTM tap)]: the units a thread of lstm_rec_any_kernel takes in its pass i, per direction."""
    return [(f"dir {d} pass {i}", slice(d * H + 256 * i, d * H + min(256 * (i + 1), H))) for d in range(D) for i in range((H + 255) // 256)]


def err(a, truth):
    return float(np.abs(a.double().cpu().numpy() - truth).max())


def rms(a, truth):
    e = np.asarray(a, np.float64) - truth
    return float(np.sqrt((e * e).mean()))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_wide_and_narrow_models_match_float64(name, mode):
    """Logits, probabilities and both taps of every case in every GEMM mode within LOGIT_TOL of float64, on a poisoned workspace; the LSTM
    tap's error per pass of the generic recurrence, so that a defect confined to one pass is named; the recurrence is the 4-sequence form
    and time chunks, asked for, do not exist at these hidden sizes."""
    F, H, L, bi, lh, ll, B, T = CASES[name]
    D = 2 if bi else 1
    truth, cpu = reference(name)
    rt = runtime(name)
    rt.set_gemm_mode(mode)
    rt.set_time_chunks(4)
    try:
        lg, pr = poisoned_classify(rt, features(name).to(DEV))
        assert rt.recurrent_tile() == 4
        assert rt.time_chunks() == 1
        y, z = rt.taps()
        torch.cuda.synchronize()
    finally:
        rt.set_time_chunks(0)
    assert lg.shape == pr.shape == (B, T) and y.shape == (B, T, H * D)
    e_lg, e_pr, e_y = err(lg, truth["logits"]), err(pr, truth["probs"]), err(y, truth["lstm"])
    e_z = err(z, truth["lin"]) if ll > 0 else 0.0
    per_pass = [(label, err(y[..., cols], truth["lstm"][..., cols])) for label, cols in passes_of(H, D)]
    worst = max(per_pass, key=lambda p: p[1] if np.isfinite(p[1]) else np.inf)
    r_gpu, r_cpu = rms(y.double().cpu().numpy(), truth["lstm"]), rms(cpu["lstm"], truth["lstm"])
    c_lg = float(np.abs(cpu["logits"] - truth["logits"]).max())
    print(f"wide {name} {mode}: logits {e_lg:.2e} probs {e_pr:.2e} lstm tap {e_y:.2e} lin tap {e_z:.2e}  "
          f"(logits {truth['logits'].min():.2f} .. {truth['logits'].max():.2f}; fp32 CPU path: logits {c_lg:.2e})")
    print(f"wide {name} {mode}: lstm tap per pass: " + ", ".join(f"{label} {e:.2e}" for label, e in per_pass) + f"; worst {worst[0]}")
    print(f"wide {name} {mode}: lstm tap rms vs float64: GPU {r_gpu:.2e} CPU {r_cpu:.2e} ratio {r_gpu / r_cpu:.2f}")
    for what, t in (("logits", lg), ("probs", pr), ("lstm tap", y)) + ((("lin tap", z),) if ll > 0 else ()):
        assert bool(torch.isfinite(t).all()), (name, mode, what)
    for label, e in per_pass:
        assert e < LOGIT_TOL, (name, mode, label, e)
    assert e_y < LOGIT_TOL and e_z < LOGIT_TOL, (name, mode, e_y, e_z)
    assert e_lg < LOGIT_TOL and e_pr < LOGIT_TOL, (name, mode, e_lg, e_pr)
    if ll == 0:
        assert z is None


@pytest.mark.parametrize("mode", ["f32", "f16p"])
@pytest.mark.parametrize("name", STRUCTURE_CASES)
def test_batch_placement_and_repetition_change_no_bit(name, mode):
    """One sequence in lane 0 and lane 3 of a full tile and in lane 0 of a partial last tile (B = 9: rows 0, 3, 8), other sequences around
    it: the three copies have the same logits, probabilities and taps bit for bit (a unit's chain depends on its own sequence only, in
    every pass), and a second run on a freshly poisoned workspace repeats every bit of the first."""
    F, H, L, bi, lh, ll, _, T = CASES[name]
    rt = runtime(name)
    rt.set_gemm_mode(mode)
    x = features(name, B=9)
    x[3] = x[0]
    x[8] = x[0]
    assert not torch.equal(x[1], x[0])
    x = x.to(DEV)
    runs = []
    for _ in range(2):
        lg, pr = poisoned_classify(rt, x)
        y, z = rt.taps()
        runs.append((lg.clone(), pr.clone(), y.clone(), z.clone()))
    for what, a, b in zip(("logits", "probs", "lstm tap", "lin tap"), runs[0], runs[1]):
        assert bool(torch.isfinite(a).all()), (name, mode, what)
        assert torch.equal(a, b), (name, mode, what, "run to run")
        for row in (3, 8):
            assert torch.equal(a[row], a[0]), (name, mode, what, row, float((a[row] - a[0]).abs().max()))
    assert not torch.equal(runs[0][0][1], runs[0][0][0])


def lens_9(T):
    """A full tile, a tile whose rows are all empty (the tmax == 0 return of the lens form), a partial one."""
    return [T, 1, 7, 0, 0, 0, 0, 0, 5]


def dense_per_length(rt, feats, lens):
    """{row: logits (len,)} from dense classify on the rows of each length at T = len (tests/test_gpu_ragged.py)."""
    out = {}
    for n in sorted(set(lens)):
        if n == 0:
            continue
        idx = [b for b, v in enumerate(lens) if v == n]
        lg, _ = poisoned_classify(rt, feats[idx, :n].contiguous())
        for k, b in enumerate(idx):
            out[b] = lg[k].clone()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", STRUCTURE_CASES)
def test_per_row_lengths_on_the_generic_recurrence(name, mode):
    """uvad_classify_lens at B = 9 with lengths T, 1, 7, 0, 0, 0, 0, 0, 5: valid frames are the dense call of each length alone (bit for bit
    in modes f32 and f16p_stream, LOGIT_TOL in f16p / f16p3, whose kernels may depend on the launch size) and within LOGIT_TOL of float64;
    outputs past a length are exactly 0; NaN and 1e30 in the padding frames change no bit."""
    from oracle import parity_stats as ps
    F, H, L, bi, lh, ll, _, T = CASES[name]
    lens = lens_9(T)
    assert max(lens) == T and all(0 <= n <= T for n in lens)
    rt = runtime(name)
    rt.set_gemm_mode(mode)
    host = features(name, B=9)
    clean = host.clone()
    for b, n in enumerate(lens):
        clean[b, n:] = 0.0
    lg, pr = poisoned_classify(rt, clean.to(DEV), lengths=lens)
    lg, pr = lg.clone(), pr.clone()
    assert rt.recurrent_tile() == 4
    assert bool(torch.isfinite(lg).all()) and bool(torch.isfinite(pr).all()), (name, mode, "non-finite output")
    want = dense_per_length(rt, clean.to(DEV), lens)
    exact = mode in ("f32", "f16p_stream")
    worst, worst64 = 0.0, 0.0
    for b, n in enumerate(lens):
        if n:
            d = float((lg[b, :n] - want[b]).abs().max())
            worst = max(worst, d)
            if exact:
                assert torch.equal(lg[b, :n], want[b]), (name, mode, b, n, d)
            t = ps.truth_logits(state_dict(name), host[b:b + 1, :n], F, H, L, bi, lh, ll)[0]
            worst64 = max(worst64, err(lg[b, :n], t))
        assert torch.count_nonzero(lg[b, n:]) == 0 and torch.count_nonzero(pr[b, n:]) == 0, (name, mode, b)
        assert not bool(torch.signbit(lg[b, n:]).any())
    print(f"wide lens {name} {mode}: max |ragged - dense| {worst:.2e} ({'bit for bit' if exact else 'LOGIT_TOL'}), vs float64 {worst64:.2e}")
    assert worst < LOGIT_TOL and worst64 < LOGIT_TOL, (name, mode, worst, worst64)
    for value in (float("nan"), 1e30):
        dirty = host.clone()
        for b, n in enumerate(lens):
            dirty[b, n:] = value
        lg2, pr2 = poisoned_classify(rt, dirty.to(DEV), lengths=lens)
        assert torch.equal(lg2, lg) and torch.equal(pr2, pr), (name, mode, value)


def test_the_acceptance_boundary_of_uvad_create():
    """hidden 1024 builds and runs; 1056, and 1040 with one direction, are refused with "multiple of 32"; lin_hidden = 6 is refused."""
    import uvad_amd
    rt = runtime("h1024-uni-lin0")
    rt.set_gemm_mode("f16p")
    lg, _ = poisoned_classify(rt, features("h1024-uni-lin0").to(DEV))
    assert bool(torch.isfinite(lg).all()) and err(lg, reference("h1024-uni-lin0")[0]["logits"]) < LOGIT_TOL

    def create(lstm, linear):
        return uvad_amd.VadRuntime(DEV, fbank=None, model={"encoding_dim": 64, "lstm": dict({"num_layers": 1, "bidirectional": True}, **lstm),
                                                           "linear": linear})
    for lstm in ({"hidden_size": 1056}, {"hidden_size": 1040, "bidirectional": False}):
        with pytest.raises(RuntimeError, match="multiple of 32"):
            create(lstm, {"hidden_size": 128, "num_layers": 2})
    with pytest.raises(RuntimeError, match="bad model configuration"):
        create({"hidden_size": 128}, {"hidden_size": 6, "num_layers": 2})
