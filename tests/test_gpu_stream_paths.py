"""uvad_stream_step: every shape a step can take, the state it hands from one shape to the next, and the isolation of a feed.

What a step launches is decided per step (csrc/uvad_api.hip: stream_uses_stack, stream_head_in_stack, lstm_stack_fb_lds_bytes, y_planes):

  A  one launch, lstm_stack_kernel<K, false, true>: feature stage, every layer, the head
  B  fbank_kernel, then lstm_stack_kernel<K, false, false> with the head inside (the feature stage does not fit beside the stack)
  C  fbank_kernel, the stack with f16 plane output <K, true, false>, then the split-f16 feed-forward GEMMs and the classifier
  D  fbank_kernel, the stack with f32 row output, then the exact-f32 feed-forward GEMMs and the classifier
  E  fbank_kernel, then projection + recurrence per layer with the carried state

with   stack = hidden 128, F in {64, 80}, 1..8 layers, k <= LSTM_STACK_TMAX = 4      (stream_uses_stack)
       head  = at most 4 feed-forward layers, each 128 -> 128                         (stream_head_in_stack)
       fits  = 4 rows of (k - 1) * 160 + 400 samples + the mel image + the transform scratch <= 120 KiB   (lstm_stack_fb_lds_bytes)
       A = stack and head and fits;  B = stack and head and not fits;  C / D = stack and not head, split-f16 modes / mode f32;
       E = not stack.
fits fails for no table FbankConfig builds (80 filters: bands of 16 bins at most, an 8 KiB image), but uvad_set_tables accepts any matrix: with one filter 160
bins wide the 80-filter image is 160 x 128 floats = 80 KiB, + 36 KiB of scratch + 6.25 KiB of samples at k = 1 > 120 KiB -> path B.

CASES below is the table: name -> configuration and the path(s) its steps take; path_of() restates the predicates and every test
checks the table against it with the k of every step, so the claims can be read against uvad_api.hip without a GPU.

Reference and bound: the offline call on the whole signal in the same GEMM mode (causal model: identical by causality), itself held
to the CPU oracle on the same features; LOGIT_TOL = 1e-4 at weights x 2 is the project's bound (tests/test_gpu_parity.py).  The
isolation, state and canary tests are bit for bit: nothing in a step couples two feeds or two state blocks.
"""
import functools

import numpy as np
import pytest
import torch

import stream_ref as sr

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
DEV = "cuda:0"
B7 = 7                      # one full 4-sequence workgroup and one with a padding sequence
ROWS = (0, 3, 4, 6)         # first and last lane of the full tile, both sides of the partial one
TMAX = 4                    # LSTM_STACK_TMAX (csrc/uvad_internal.h)


def cfg(paths, chunk, F=64, window="povey", layers=4, hidden=128, lin=(128, 2), slope=0.01, mode="f16p", B=B7, seconds=1.0, wide_mel=False):
    return dict(paths=paths, chunk=chunk, F=F, window=window, layers=layers, hidden=hidden, lin=lin, slope=slope, mode=mode, B=B,
                seconds=seconds, wide_mel=wide_mel)


CASES = {
    # ---- A: stack, head and feature stage in one launch.  chunk 160 / 320 / 480 / 640 -> k = 1 / 2 / 3 / 4 (first step: 0 / 1 / 2 / 3)
    "A-f64-l1-ff2-c160": cfg("A", 160, layers=1),
    "A-f64-l4-ff0-c320": cfg("A", 320, lin=(128, 0)),
    "A-f64-l8-ff4-c640": cfg("A", 640, layers=8, lin=(128, 4)),
    "A-f64-l4-ff1-c480-slope": cfg("A", 480, lin=(128, 1), slope=0.2),
    "A-f80-l1-ff4-c480": cfg("A", 480, F=80, window="hamming", layers=1, lin=(128, 4)),
    "A-f80-l4-ff2-c640": cfg("A", 640, F=80, window="hamming"),
    "A-f80-l8-ff0-c160": cfg("A", 160, F=80, window="hamming", layers=8, lin=(128, 0)),
    "A-f80-l4-ff1-c320": cfg("A", 320, F=80, window="hamming", lin=(128, 1)),
    # ---- B: as A, but the mel image of a 160-bin filter leaves no room for the feature stage (fits = false at every k)
    "B-f80-widemel-c640": cfg("B", 640, F=80, window="hamming", wide_mel=True),
    "B-f80-widemel-c320": cfg("B", 320, F=80, window="hamming", layers=2, wide_mel=True),
    # ---- C / D: head = false (64-wide feed-forward layers; five of them): plane output + split-f16 head, f32 rows + exact head
    **{f"{'D' if mode == 'f32' else 'C'}-f{F}-lin{lin[0]}x{lin[1]}-{mode}-c{chunk}":
       cfg("D" if mode == "f32" else "C", chunk, F=F, window="povey" if F == 64 else "hamming", layers=layers, lin=lin, mode=mode)
       for (F, lin, layers, chunk) in ((64, (64, 2), 4, 320), (80, (64, 2), 4, 640), (64, (128, 5), 2, 640), (80, (128, 5), 2, 480))
       for mode in ("f16p", "f16p3", "f16p_stream", "f32")},
    # ---- C with rows past one 128-row plane tile: 10 workgroups x 4 frames x 4 sequences = 160 rows
    "C-f64-lin64x2-f16p-c640-B40": cfg("C", 640, lin=(64, 2), B=40),
    # ---- E: stack = false, one reason each: k = 5; F = 40; hidden 64; 9 layers
    "E-k5-c800": cfg("AE", 800),                  # (its first step has k = 4: A; every other one k = 5)
    "E-k5-c800-f32": cfg("AE", 800, mode="f32"),
    "E-f40-c320": cfg("E", 320, F=40),
    "E-h64-c320": cfg("E", 320, hidden=64),
    "E-l9-c320": cfg("E", 320, layers=9),
    # ---- E on the generic recurrence (hidden not 128 / 64): (h, c) updated in place by lstm_rec_any_kernel, two passes / three passes / 32 units
    "E-h288-c320": cfg("E", 320, hidden=288, layers=2, lin=(100, 2)),
    "E-h544-c480-f32": cfg("E", 480, hidden=544, layers=2, mode="f32"),
    "E-h32-c160": cfg("E", 160, hidden=32, layers=3, lin=(36, 2)),
    # ---- mixed sessions: the two kernels take turns on one (h, c) block and one PCM tail
    "mixed-AE-c700": cfg("AE", 700, seconds=1.5),
    "mixed-AE-f80-c700": cfg("AE", 700, F=80, window="hamming", seconds=1.5),
    "mixed-CE-c700": cfg("CE", 700, lin=(64, 2), seconds=1.5),
    "mixed-DE-c700": cfg("DE", 700, lin=(64, 2), mode="f32", seconds=1.5),
    "mixed-A-k34-c560": cfg("A", 560, seconds=1.5),       # k = 3 / 4 alternating: odd and even frame pairing inside the fused feature stage
    "mixed-A-k0-first-c160": cfg("A", 160, layers=2),     # first step without a frame: the staging kernel writes the tail
}


@functools.lru_cache(maxsize=None)
def mel_stride(F, wide):
    """The longest band of the mel matrix in bins, rounded up to a multiple of 4 (uvad_set_tables)."""
    import uvad_amd
    mel = wide_mel_matrix() if wide else uvad_amd.make_mel_matrix(F, 512, 16000, 20.0, -400.0)
    longest = max(int(np.flatnonzero(row)[-1] - np.flatnonzero(row)[0] + 1) for row in mel if row.any())
    return (longest + 3) // 4 * 4


def predicates(c, k):
    """(stack, head, fits) of csrc/uvad_api.hip for a step of k > 0 frames of configuration c: stream_uses_stack(c, k),
    stream_head_in_stack(c), lstm_stack_fb_lds_bytes(fa, k) > 0."""
    stack = c["hidden"] == 128 and c["F"] in (64, 80) and 1 <= k <= TMAX and 1 <= c["layers"] <= 8
    head = c["lin"][1] <= 4 and (c["lin"][1] == 0 or c["lin"][0] == 128)
    image = mel_stride(c["F"], c["wide_mel"]) * (64 if c["F"] <= 64 else 128)      # floats: [bin in band][64 or 128 filter columns]
    rows = 4 * (((k - 1) * 160 + 400 + 3) // 4 * 4)                                 # the workgroup's 4 rows of samples
    fits = 4 * (rows + image + 8 * 2 * 576) <= 120 * 1024                           # + the transform scratch of 8 waves
    return stack, head, fits


def path_of(c, k):
    stack, head, fits = predicates(c, k)
    if not stack:
        return "E"
    if not head:
        return "D" if c["mode"] == "f32" else "C"
    return "A" if fits else "B"


def steps_of(c):
    return int(c["seconds"] * 16000) // c["chunk"]


def check_paths(c, ks):
    assert ks == sr.k_schedule(c["chunk"], len(ks)), (ks, sr.k_schedule(c["chunk"], len(ks)))
    assert {path_of(c, k) for k in ks if k > 0} == set(c["paths"]), (c["paths"], ks)


@functools.lru_cache(maxsize=None)
def pcm(B, S):
    from uvad_amd.synth import synth_pcm
    return torch.from_numpy(synth_pcm(B, S, seed=4100)).to(DEV)


def state_dict(c):
    from oracle import torch_ref as tr
    return tr.seeded_state_dict(c["F"], c["hidden"], c["layers"], False, c["lin"][0], c["lin"][1], seed=1234, scale=2.0)


def wide_mel_matrix():
    import uvad_amd
    mel = uvad_amd.make_mel_matrix(80, 512, 16000, 20.0, -400.0)
    bins = np.arange(96, 256)                       # one filter 160 bins wide (a triangle over 3 .. 8 kHz): mel_stride = 160
    mel[79] = 0.0
    mel[79, bins] = (1.0 - np.abs(bins - 175.5) / 80.0).astype(np.float32)
    assert (mel[79, bins] > 0).all()
    return mel


_RUNTIMES = {}


def runtime(c, fresh=False):
    """The VadRuntime of a configuration (kept for the module: the tests of one path share it), in the configuration's GEMM mode."""
    import uvad_amd
    key = (c["F"], c["window"], c["layers"], c["hidden"], c["lin"], c["slope"], c["wide_mel"])
    rt = None if fresh else _RUNTIMES.get(key)
    if rt is None:
        model = {"encoding_dim": c["F"], "lstm": {"hidden_size": c["hidden"], "num_layers": c["layers"], "bidirectional": False},
                 "linear": {"hidden_size": c["lin"][0], "num_layers": c["lin"][1]}, "leaky_slope": c["slope"]}
        rt = uvad_amd.VadRuntime(DEV, fbank=uvad_amd.FbankConfig(num_filters=c["F"], window_type=c["window"]), model=model)
        if c["wide_mel"]:
            rt.set_tables(uvad_amd.make_window(c["window"], 400), wide_mel_matrix())
        rt.load_state_dict(state_dict(c))
        if not fresh:
            _RUNTIMES[key] = rt
    rt.set_gemm_mode(c["mode"])
    return rt


def session(rt, x, chunk, steps, st=None):
    """Feed x (B, >= steps * chunk) chunk by chunk: (logits of every emitted frame (B, n), the k of every step, the session)."""
    st = st if st is not None else rt.stream_open(x.shape[0], chunk)
    outs, ks = [], []
    for i in range(steps):
        o = rt.stream_step(st, x[:, i * chunk:(i + 1) * chunk].contiguous())
        ks.append(int(o.shape[1]))
        outs.append(o.clone())
    return torch.cat(outs, dim=1), ks, st


def reset(rt, st):
    rt._check(rt.lib.uvad_stream_reset(rt.ctx, st["state"].data_ptr(), st["B"], rt._stream()))


_CLEAN = {}


def clean_session(name):
    """The B = 7 session of a case on its cached runtime (shared, never modified)."""
    if name not in _CLEAN:
        c = CASES[name]
        got, ks, _ = session(runtime(c), pcm(c["B"], steps_of(c) * c["chunk"]), c["chunk"], steps_of(c))
        check_paths(c, ks)
        _CLEAN[name] = (got, ks)
    return _CLEAN[name]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. every dispatch path against the reference, frame for frame
@pytest.mark.parametrize("name", list(CASES))
def test_every_path_equals_offline_and_the_oracle_frame_for_frame(name):
    """Every emitted frame of every feed: the k of every step is the brute-force schedule, the steps take the paths the table claims
    (path_of: the predicates of uvad_api.hip), |stream - offline| < LOGIT_TOL in the same GEMM mode, and the offline logits are within
    LOGIT_TOL of the CPU oracle on the same features (uvad_fbank's) and weights."""
    from oracle import c_oracle as co
    c = CASES[name]
    rt = runtime(c)
    steps, chunk, B = steps_of(c), c["chunk"], c["B"]
    x = pcm(B, steps * chunk)
    got, ks = clean_session(name) if B == B7 else session(rt, x, chunk, steps)[:2]
    check_paths(c, ks)
    rt.set_gemm_mode(c["mode"])
    offline, _ = rt.forward(x)
    n = got.shape[1]
    assert n == sum(ks) == sr.frames_complete(steps * chunk) and n <= offline.shape[1] and got.shape[0] == B
    assert torch.isfinite(got).all() and torch.isfinite(offline).all()
    e_stream = float((got - offline[:, :n]).abs().max())
    sd = {k: v.numpy() for k, v in state_dict(c).items()}
    mc = co.ModelCfg(c["F"], c["hidden"], c["layers"], 0, c["lin"][0], c["lin"][1], c["slope"])
    want, _ = co.classify(sd, mc, rt.fbank(x).cpu().numpy())
    e_oracle = float(np.abs(offline.cpu().numpy() - want).max())
    why = {k: "".join(n if p else "-" for n, p in zip("SHF", predicates(c, k))) for k in sorted(set(ks)) if k > 0}
    print(f"stream paths {name}: paths {c['paths']} (stack / head / fits by k: {why}) frames {n} x {B}: |stream - offline| {e_stream:.2e}  "
          f"|offline - oracle| {e_oracle:.2e}  (logits {want.min():.2f} .. {want.max():.2f})")
    assert e_stream < LOGIT_TOL, (name, e_stream)
    assert e_oracle < LOGIT_TOL, (name, e_oracle)


def state_layout(rt, c, B):
    """(bytes of the two PCM tails, bytes of one layer's h or c) of a state block: tail[2][B][400] f32 | h per layer | c per layer,
    every block 256-aligned (stream_layout in csrc/uvad_api.hip); checked against uvad_stream_state_bytes."""
    al = lambda n: (n + 255) // 256 * 256
    tails, stride = 2 * al(B * 400 * 4), al((B + 3) // 4 * 4 * c["hidden"] * 4)
    assert tails + 2 * c["layers"] * stride == int(rt.lib.uvad_stream_state_bytes(rt.ctx, B))
    return tails, stride


@pytest.mark.parametrize("name", ["A-f64-l8-ff4-c640", "A-f80-l8-ff0-c160", "mixed-AE-c700", "C-f64-lin64x2-f16p-c320", "E-l9-c320"])
def test_the_bound_sees_the_loss_of_any_carried_block(name):
    """The control of the test above: how far is LOGIT_TOL from what a hand-off fault would do?  Half way through the session ONE
    block of the carried state is zeroed -- the (h, c) of one layer, for every layer in turn, then the two PCM tails.  Every frame
    emitted before keeps its bits and the frames after move by more than LOGIT_TOL, also in the 8- and 9-layer models whose
    logits span a few hundredths only: a step that lost or misplaced any of these blocks could not pass the comparison with
    the offline call."""
    c = CASES[name]
    rt = runtime(c)
    steps, chunk = steps_of(c), c["chunk"]
    x = pcm(B7, steps * chunk)
    clean, ks = clean_session(name)
    tails, stride = state_layout(rt, c, B7)
    half = steps // 2
    done = sum(ks[:half])
    blocks = {f"layer {l}": [(tails + l * stride, stride), (tails + (c["layers"] + l) * stride, stride)] for l in range(c["layers"])}
    blocks["tails"] = [(0, tails)]
    for what, spans in blocks.items():
        st = rt.stream_open(B7, chunk)
        outs = []
        for i in range(steps):
            if i == half:
                for o, nbytes in spans:
                    st["state"][o:o + nbytes] = 0
            outs.append(rt.stream_step(st, x[:, i * chunk:(i + 1) * chunk].contiguous()).clone())
        got = torch.cat(outs, dim=1)
        dev = float((got[:, done:] - clean[:, done:]).abs().max())
        print(f"lost state {name}: {what} zeroed before step {half}: later frames move by {dev:.2e}")
        assert torch.equal(got[:, :done], clean[:, :done])
        assert dev > LOGIT_TOL, (name, what, dev)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. a feed depends on nothing but its own samples
ISOLATION = {
    # name of the case -> bit for bit?  (the per-layer kernels of path E are held launch-size independent in modes f32 and f16p_stream
    # by tests/test_gpu_window_slots.py; in f16p and f16p3 the bound is LOGIT_TOL)
    "A-f64-l8-ff4-c640": True, "A-f80-l4-ff2-c640": True, "B-f80-widemel-c640": True,
    "C-f64-lin64x2-f16p-c320": True, "C-f80-lin64x2-f16p3-c640": True, "C-f64-lin128x5-f16p_stream-c640": True,
    "D-f64-lin64x2-f32-c320": True, "D-f80-lin128x5-f32-c480": True,
    "mixed-AE-c700": False, "mixed-DE-c700": True,
    "E-k5-c800": False, "E-k5-c800-f32": True,
}
ISOLATION_MODES = {"E-k5-c800": ("f16p", "f16p3", "f16p_stream"), "mixed-AE-c700": ("f16p", "f16p_stream")}


@pytest.mark.parametrize("name", list(ISOLATION))
def test_a_feed_of_seven_equals_the_same_feed_alone(name):
    """Row b of the B = 7 session against the B = 1 session fed row b alone, b in {0, 3, 4, 6}.  The stack kernel's chains never mix
    the four B-operand columns of v_mfma_f32_4x4x1 and the GEMMs of the heads never mix rows: bit for bit on paths A, B, C, D and on
    E in the modes whose kernels do not depend on the launch size (f32, f16p_stream); LOGIT_TOL on E in f16p / f16p3."""
    base = CASES[name]
    for mode in ISOLATION_MODES.get(name, (base["mode"],)):
        c = dict(base, mode=mode)
        exact = ISOLATION[name] or mode in ("f32", "f16p_stream")
        rt = runtime(c)
        steps, chunk = steps_of(c), c["chunk"]
        x = pcm(B7, steps * chunk)
        got, ks, _ = session(rt, x, chunk, steps)
        check_paths(c, ks)
        worst = 0.0
        for b in ROWS:
            alone, ks1, _ = session(rt, x[b:b + 1], chunk, steps)
            assert ks1 == ks
            worst = max(worst, float((alone[0] - got[b]).abs().max()))
            if exact:
                assert torch.equal(alone[0], got[b]), (name, mode, b, worst)
        print(f"feed isolation {name} mode {mode}: worst |B=7 row - B=1| {worst:.2e} ({'bit for bit' if exact else 'LOGIT_TOL'})")
        assert worst < LOGIT_TOL


# ------------------------------------------------------------------------------------------------------------------------------
# 3. state blocks are independent; reset restarts
def test_two_interleaved_sessions_equal_their_own_runs():
    """Two state blocks on one context, B = 7 / chunk 320 (path A) and B = 5 / chunk 700 (A and E), stepped in turns: each gives the bits
    of its own uninterleaved run (the counters live in the context, keyed by the state pointer)."""
    c = CASES["mixed-AE-c700"]
    rt = runtime(c)
    n1, n2 = 40, 20
    x1, x2 = pcm(B7, n1 * 320), pcm(5, n2 * 700) * 0.5
    want1, ks1, _ = session(rt, x1, 320, n1)
    want2, ks2, _ = session(rt, x2, 700, n2)
    assert set(ks2) == {3, 4, 5} and set(ks1) == {1, 2}
    s1, s2 = rt.stream_open(B7, 320), rt.stream_open(5, 700)
    o1, o2 = [], []
    for i in range(n1):
        o1.append(rt.stream_step(s1, x1[:, i * 320:(i + 1) * 320].contiguous()).clone())
        if i % 2 == 1:
            j = i // 2
            o2.append(rt.stream_step(s2, x2[:, j * 700:(j + 1) * 700].contiguous()).clone())
    assert [o.shape[1] for o in o1] == ks1 and [o.shape[1] for o in o2] == ks2
    assert torch.equal(torch.cat(o1, 1), want1) and torch.equal(torch.cat(o2, 1), want2)


@pytest.mark.parametrize("name", ["A-f64-l8-ff4-c640", "C-f64-lin64x2-f16p-c320", "mixed-AE-c700"])
def test_reset_and_a_late_first_step_give_the_bits_of_a_fresh_session(name):
    """uvad_stream_reset on a used state block, then the same audio: the bits of the first run.  And a state block stepped for the
    first time after another one on the same context has advanced through a whole session: the bits of a fresh runtime."""
    c = CASES[name]
    steps, chunk = steps_of(c), c["chunk"]
    x = pcm(B7, steps * chunk)
    want, ks = clean_session(name)
    rt = runtime(c)
    other = pcm(B7, steps * chunk).flip(0) * 0.7
    got, _, st = session(rt, other, chunk, steps)             # the block sees other audio first
    assert not torch.equal(got, want)
    reset(rt, st)
    again, ks2, _ = session(rt, x, chunk, steps, st=st)
    assert ks2 == ks and torch.equal(again, want)
    fresh = runtime(c, fresh=True)
    try:
        late = fresh.stream_open(B7, chunk)                   # opened first, stepped after another session has run to its end
        session(fresh, other, chunk, steps)
        got, ks3, _ = session(fresh, x, chunk, steps, st=late)
        assert ks3 == ks and torch.equal(got, want)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. a non-finite sample stays in its feed
@pytest.mark.parametrize("sample", [8000, 8160])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ["A-f64-l8-ff4-c640", "C-f64-lin64x2-f16p-c320", "mixed-AE-c700"])
def test_a_non_finite_sample_poisons_its_own_feed_only(name, value, sample):
    """One NaN / +Inf sample in feed 5 (the partial workgroup's second lane).  Feeds 0-4 and 6 keep every bit.  Feed 5 is non-finite
    from the first frame t0 whose 400-sample span holds the sample (49 for sample 8000, 50 for 8160) and for every frame after it: the
    frame's energies are NaN, the floor keeps NaN as the reference's clamp does, tanh_f carries it into (h, c) and the state stays
    poisoned as torch's CPU LSTM would.  Before that, feed 5 keeps every bit.

    One step earlier by design where t0 is the SECOND frame of a pair: the feature stage transforms the frames at positions (2i, 2i + 1)
    of a step through one complex FFT (csrc/fbank_pair.h), so frame t0 - 1, completed by the same chunk and emitted by the same step,
    shares the transform and its energies are NaN too.  Sample 8000 puts t0 at an even position of its step on all three paths
    (strict: nothing earlier than t0), sample 8160 at an odd one (t0 - 1, never earlier).  After uvad_stream_reset the block gives
    clean bits again."""
    c = CASES[name]
    steps, chunk = steps_of(c), c["chunk"]
    clean, ks = clean_session(name)
    n = clean.shape[1]
    t0 = sr.frames_covering(sample, n)[0]
    assert t0 == (49 if sample == 8000 else 50)
    pos = sr.step_and_position(ks, t0)[1]
    assert pos % 2 == (0 if sample == 8000 else 1), (ks, t0, pos)
    onset = t0 - (pos & 1)
    rt = runtime(c)
    x = pcm(B7, steps * chunk).clone()
    x[5, sample] = value
    got, ks2, st = session(rt, x, chunk, steps)
    assert ks2 == ks
    others = [0, 1, 2, 3, 4, 6]
    assert torch.equal(got[others], clean[others])
    bad = ~torch.isfinite(got[5])
    first_bad = int(bad.nonzero()[0]) if bad.any() else -1
    print(f"non-finite {name} {value} at sample {sample}: t0 {t0} (position {pos} of its step), feed 5 non-finite from frame {first_bad}, "
          f"{int(bad.sum())} of {n} frames")
    assert first_bad == onset and bool(bad[onset:].all()) and not bool(bad[:onset].any())
    assert torch.equal(got[5, :onset], clean[5, :onset])
    reset(rt, st)
    again, _, _ = session(rt, pcm(B7, steps * chunk), chunk, steps, st=st)
    assert torch.equal(again, clean)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. nothing written that was not promised
CANARY = int(np.array([0xCAFEF00D], np.uint32).view(np.int32)[0])


def raw_step(rt, st, chunk_pcm, out, ld):
    return int(rt.lib.uvad_stream_step(rt.ctx, chunk_pcm.data_ptr(), st["B"], st["chunk"], st["state"].data_ptr(), out.data_ptr(), ld,
                                       st["ws"].data_ptr(), st["ws"].numel(), rt._stream()))


@pytest.mark.parametrize("name", ["A-f64-l8-ff4-c640", "mixed-A-k0-first-c160", "C-f64-lin64x2-f16p-c640-B40", "C-f80-lin64x2-f16p-c640",
                                  "E-k5-c800", "mixed-AE-c700"])
def test_a_step_writes_k_columns_of_b_rows_and_nothing_else(name):
    """uvad_stream_step on a (B + 1) x (k_max + 3) output pre-filled with a canary: after every step the columns >= k of the B rows
    and the whole extra row still hold it, the k columns are the bits the public session gives, and a step without a frame writes
    nothing."""
    c = CASES[name]
    rt = runtime(c)
    steps, chunk, B = steps_of(c), c["chunk"], c["B"]
    x = pcm(B, steps * chunk)
    want, ks = clean_session(name) if B == B7 else session(rt, x, chunk, steps)[:2]
    check_paths(c, ks)
    ld = chunk // 160 + 1 + 3
    st = rt.stream_open(B, chunk)
    out = torch.empty((B + 1, ld), dtype=torch.int32, device=DEV)
    done = 0
    for i in range(steps):
        out.fill_(CANARY)
        k = raw_step(rt, st, x[:, i * chunk:(i + 1) * chunk].contiguous(), out, ld)
        torch.cuda.synchronize()
        assert k == ks[i], (i, k, ks[i])
        assert bool((out[:B, k:] == CANARY).all()) and bool((out[B] == CANARY).all()), (name, i, k)
        assert torch.equal(out[:B, :k].view(torch.float32), want[:, done:done + k]), (name, i)
        done += k
    assert 0 in ks or name != "mixed-A-k0-first-c160"
    assert done == want.shape[1]


@pytest.mark.parametrize("name", ["A-f64-l8-ff4-c640", "E-k5-c800"])
def test_a_short_output_row_is_refused_and_the_step_can_be_repeated(name):
    """ld_logits < k: UVAD_E_ARG, nothing written, and the session has not moved: the same chunk with room for its frames gives the
    bits of an undisturbed session (path A: first step, k = 3; path E: second step, k = 5)."""
    c = CASES[name]
    rt = runtime(c)
    chunk = c["chunk"]
    x = pcm(B7, steps_of(c) * chunk)
    want, ks = clean_session(name)
    ld = chunk // 160 + 1
    st = rt.stream_open(B7, chunk)
    out = torch.empty((B7 + 1, ld), dtype=torch.int32, device=DEV)
    done = 0
    for i in range(3):
        xi = x[:, i * chunk:(i + 1) * chunk].contiguous()
        if (name[0] == "A" and i == 0) or (name[0] == "E" and i == 1):
            out.fill_(CANARY)
            assert raw_step(rt, st, xi, out, ks[i] - 1) == -1                      # UVAD_E_ARG
            assert b"ld_logits" in rt.lib.uvad_last_error(rt.ctx)
            torch.cuda.synchronize()
            assert bool((out == CANARY).all())
        assert raw_step(rt, st, xi, out, ld) == ks[i]
        assert torch.equal(out[:B7, :ks[i]].view(torch.float32), want[:, done:done + ks[i]]), (name, i)
        done += ks[i]
