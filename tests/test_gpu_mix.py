"""The noise-mixing stage on the device (uvad_mix_*, include/uvad.h) against tests/mix_ref.py: plan byte for byte, energies, gains and
output bit for bit, f32 and int16, in place and out of place, with canaries around every buffer the calls write and NaN past every
length; the draw ordinal, graph replay, independence of the batch, the refusals; then the host layer (mix_open / mix_step)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mix_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG, E_STATE = -1, -3
B, S = 5, 1030                                   # rows 1 and 3 start 8 bytes off a 16-byte boundary
LENS = [1030, 0, 1, 257, 1027]
CLIPS = [1, 3, 257, 1000, 4099, 64]              # clip 2 is all zeros
SEED, Q, MAX_SEG = 0x1234567887654321, 16, 8
GUARD = 256                                      # canary bytes on both sides of a guarded buffer


@pytest.fixture(scope="module")
def rt():
    from uvad_amd.runtime import VadRuntime
    r = VadRuntime(DEV)                          # no feature tables, weights or model
    yield r
    r.close()


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((B, S)) * 0.1).astype(np.float32)
    x[0, 5] = -0.0
    q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    first = np.zeros(len(CLIPS) + 1, np.int64)
    first[1:] = np.cumsum(CLIPS)
    bank = (rng.standard_normal(int(first[-1])) * 0.3).astype(np.float32)
    bank[first[2]:first[3]] = 0.0
    xn = x.copy()
    for b, n in enumerate(LENS):                 # nothing past a length may be read
        xn[b, n:] = np.nan
        q[b, n:] = 32767
    amp = mr.amp_table(10, 20, Q)
    return {"x": xn, "q": q, "bank": bank, "first": first, "amp": amp, "e_clips": mr.clip_energies(bank, first)}


class Guarded:
    """nbytes of device memory between two canary blocks."""

    def __init__(self, nbytes, fill=0):
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.body()[:] = fill
        assert self.ptr % 256 == 0

    def body(self):
        return self.t[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD

    def put(self, a):
        self.body()[:] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)

    def get(self, dtype):
        return self.body().cpu().numpy().view(dtype).copy()

    def intact(self):
        t = self.t.cpu().numpy()
        return bool((t[:GUARD] == 0xA5).all() and (t[GUARD + self.n:] == 0xA5).all())


def _cfg(built, amp, mix_prob=0.5, max_seg=MAX_SEG, seed=SEED):
    return built.MixCfg(float(mix_prob), len(amp), amp.ctypes.data_as(C.POINTER(C.c_double)), int(max_seg), seed)


class Dev:
    """One reset state with guarded buffers, driven through the C ABI."""

    def __init__(self, rt, case, mix_prob=0.5, max_seg=MAX_SEG, bank=None, first=None, rows=B, samples=S):
        from uvad_amd import _lib
        self.lib, self.ctx, self.L = rt.lib, rt.ctx, _lib
        self.amp = case["amp"]
        self.max_seg, self.rows, self.samples = max_seg, rows, samples
        self.first = np.ascontiguousarray(case["first"] if first is None else first, np.int64)
        self.bank_host = case["bank"] if bank is None else bank
        self.bank = Guarded(4 * len(self.bank_host))
        self.bank.put(self.bank_host)
        self.cfg = _cfg(_lib, self.amp, mix_prob, max_seg)
        self.n_clips = len(self.first) - 1
        self.state = Guarded(self.lib.uvad_mix_state_bytes(C.byref(self.cfg), self.n_clips))
        self.ws = Guarded(self.lib.uvad_mix_ws_bytes(rows, max_seg))
        self.pw = 4 + 4 * max_seg
        self.plan = Guarded(4 * rows * self.pw, fill=0x77)
        self.out = Guarded(4 * rows * samples, fill=0x77)
        assert self.state.n > 0 and self.ws.n > 0
        assert self.reset() == 0, self.err()

    def err(self):
        return self.lib.uvad_last_error(self.ctx).decode()

    def reset(self):
        return self.lib.uvad_mix_reset(self.ctx, self.state.ptr, self.state.n, C.byref(self.cfg), self.bank.ptr,
                                       self.first.ctypes.data_as(C.POINTER(C.c_int64)), self.n_clips, None)

    def call(self, d_in, fmt, nsamp, draw=None, row0=0, out=None, rows=None, plan=True, stream=None):
        rows = self.rows if rows is None else rows
        head = (self.ctx, d_in, fmt, rows, self.samples, nsamp, self.out.ptr if out is None else out, self.plan.ptr if plan else None)
        tail = (self.state.ptr, self.state.n, self.ws.ptr, self.ws.n, stream)
        if draw is None:
            return self.lib.uvad_mix_step(*head, *tail)
        return self.lib.uvad_mix_apply(*head, row0, draw, *tail)

    def draws(self):
        return int(self.state.get(np.uint64)[7])

    def e_clips(self):
        off = 256 + (8 * (self.n_clips + 1) + 255) // 256 * 256
        return self.state.get(np.uint8)[off:off + 8 * self.n_clips].view(np.float64)

    def e_rows(self, rows=None):
        return self.ws.get(np.uint8)[256:256 + 8 * (self.rows if rows is None else rows)].view(np.float64)

    def intact(self):
        return all(g.intact() for g in (self.bank, self.state, self.ws, self.plan, self.out))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def dev(rt, case):
    return Dev(rt, case)


@pytest.fixture(scope="module")
def nsamp():
    return torch.tensor(LENS, dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module")
def ref(case):
    """The restatement of draws 0 .. 2 for both sample types, computed once."""
    out = {}
    for name in ("x", "q"):
        for draw in range(3):
            out[name, draw] = mr.mix(case[name], LENS, case["bank"], case["first"], case["amp"], 0.5, MAX_SEG, SEED, draw, e_clips=case["e_clips"])
    rows = [r for d in range(3) for r in out["x", d]["rows"]]
    assert any(r["mixed"] for r in rows) and not all(r["mixed"] for r in rows)            # both kinds of row are covered
    assert any(len(r["segs"]) > 1 for r in rows) and any(c == 2 for r in rows for c, *_ in r["segs"])   # several segments; the silent clip
    return out


def test_reset_computes_clip_energies_bit_for_bit(dev, case):
    torch.cuda.synchronize()
    got = dev.e_clips()
    print("clip energies", got, case["e_clips"])
    assert got[2] == 0.0 and np.array_equal(got.view(np.uint64), case["e_clips"].view(np.uint64))
    hd = dev.state.get(np.uint8)[:64]
    assert tuple(hd[4:16].view(np.int32)) == (len(CLIPS), Q, MAX_SEG) and int(hd[16:24].view(np.uint64)[0]) == 1 << 31
    assert int(hd[24:32].view(np.uint64)[0]) == SEED and int(hd[32:40].view(np.int64)[0]) == sum(CLIPS) and dev.draws() == 0
    assert dev.intact()


@pytest.mark.parametrize("kind", ["f32", "f32_in_place", "i16"])
def test_apply_matches_the_restatement(dev, case, ref, nsamp, kind):
    name, fmt = ("q", dev.L.INGEST_I16) if kind == "i16" else ("x", dev.L.INGEST_F32)
    src = Guarded(case[name].nbytes)
    for draw in range(3):
        want = ref[name, draw]
        dev.plan.body()[:] = 0x77
        dev.out.body()[:] = 0x77
        if kind == "f32_in_place":
            dev.out.put(case["x"])
            assert dev.call(dev.out.ptr, fmt, nsamp.data_ptr(), draw=draw) == 0, dev.err()
        else:
            src.put(case[name])
            assert dev.call(src.ptr, fmt, nsamp.data_ptr(), draw=draw) == 0, dev.err()
        torch.cuda.synchronize()
        plan = dev.plan.get(np.int32).reshape(B, dev.pw)
        e_rows = dev.e_rows()
        gd = np.array([g for r in mr.unpack_plan(plan) for *_, g in r["segs"]], np.float32)
        gw = np.array([g for r in want["rows"] for *_, g in r["segs"]], np.float32)
        print(kind, draw, "row energies", e_rows, "gains", gd, "restated", gw)
        assert np.array_equal(e_rows.view(np.uint64), want["e_rows"].view(np.uint64))
        assert np.array_equal(_bits(gd), _bits(gw))                  # double division and square root are correctly rounded on the device
        assert plan.tobytes() == want["plan"].tobytes()
        got = dev.out.get(np.float32).reshape(B, S)
        assert np.array_equal(_bits(got), _bits(want["out"]))
        assert src.intact() and dev.intact() and dev.draws() == 0    # apply: no state update
        for b, n in enumerate(LENS):
            assert not _bits(got[b, n:]).any()                       # +0 past a length: the NaN / 32767 there reached nothing


def test_mix_prob_zero_copies_the_bits_and_still_advances(rt, case, nsamp):
    d = Dev(rt, case, mix_prob=0.0)
    x = case["x"].copy()
    x[0, 7] = np.float32(np.nan)
    x[0, 9] = -0.0
    src = Guarded(x.nbytes)
    src.put(x)
    for i in range(2):
        assert d.call(src.ptr, d.L.INGEST_F32, None) == 0, d.err()
    torch.cuda.synchronize()
    got = d.out.get(np.float32).reshape(B, S)
    assert np.array_equal(_bits(got), _bits(x)) and d.draws() == 2 and d.intact()
    assert not d.plan.get(np.int32).reshape(B, d.pw)[:, [0, 2]].any()


def test_mix_prob_one_one_short_segment_leaves_the_rest_clean(rt, case, nsamp):
    first = np.array([0, 3, 67], np.int64)                       # clips of 3 and 64 samples
    bank = case["bank"][:67].copy() + np.float32(0.5)
    d = Dev(rt, case, mix_prob=1.0, max_seg=1, bank=bank, first=first)
    src = Guarded(case["x"].nbytes)
    src.put(case["x"])
    assert d.call(src.ptr, d.L.INGEST_F32, nsamp.data_ptr(), draw=5) == 0, d.err()
    torch.cuda.synchronize()
    want = mr.mix(case["x"], LENS, bank, first, case["amp"], 1.0, 1, SEED, 5)
    got, plan = d.out.get(np.float32).reshape(B, S), d.plan.get(np.int32).reshape(B, d.pw)
    assert plan.tobytes() == want["plan"].tobytes() and np.array_equal(_bits(got), _bits(want["out"])) and d.intact()
    for b, n in enumerate(LENS):
        assert plan[b, 0] == 1 and plan[b, 2] == (1 if n else 0)
        c = int(plan[b, 6])
        assert c <= 64 and np.array_equal(_bits(got[b, c:n]), _bits(case["x"][b, c:n]))     # the uncovered rest is clean
        if n > 1:
            assert not np.array_equal(_bits(got[b, :c]), _bits(case["x"][b, :c]))


def test_cap_holds_with_the_one_sample_clip(rt, case, nsamp):
    first = np.array([0, 1], np.int64)
    bank = np.array([0.25], np.float32)
    d = Dev(rt, case, mix_prob=1.0, max_seg=64, bank=bank, first=first)
    src = Guarded(case["x"].nbytes)
    src.put(case["x"])
    assert d.call(src.ptr, d.L.INGEST_F32, nsamp.data_ptr(), draw=0) == 0, d.err()
    torch.cuda.synchronize()
    want = mr.mix(case["x"], LENS, bank, first, case["amp"], 1.0, 64, SEED, 0)
    got, plan = d.out.get(np.float32).reshape(B, S), d.plan.get(np.int32).reshape(B, d.pw)
    assert list(plan[:, 2]) == [min(n, 64) for n in LENS]
    assert plan.tobytes() == want["plan"].tobytes() and np.array_equal(_bits(got), _bits(want["out"])) and d.intact()
    assert np.array_equal(_bits(got[0, 64:]), _bits(case["x"][0, 64:]))


def test_achieved_snr_is_the_table_entry(dev, case, nsamp):
    src = Guarded(case["x"].nbytes)
    src.put(case["x"])
    seen = 0
    for draw in range(3):
        assert dev.call(src.ptr, dev.L.INGEST_F32, nsamp.data_ptr(), draw=draw) == 0, dev.err()
        torch.cuda.synchronize()
        e_rows, e_clips = dev.e_rows(), dev.e_clips()
        for b, r in enumerate(mr.unpack_plan(dev.plan.get(np.int32).reshape(B, dev.pw))):
            for clip, _, _, g in r["segs"]:
                if e_clips[clip] == 0.0 or e_rows[b] == 0.0:
                    assert _bits(np.float32(g)) == 0
                    continue
                got = 10 * math.log10(e_rows[b] / (float(g) ** 2 * e_clips[clip]))
                want = -20 * math.log10(case["amp"][r["q"]])
                print("snr", draw, b, clip, got, want)
                assert abs(got - want) < 1e-6 and 10 < want < 20
                seen += 1
    assert seen >= 3


def test_apply_repeats_and_steps_follow_the_ordinal(rt, case, ref, nsamp):
    d = Dev(rt, case)
    src = Guarded(case["x"].nbytes)
    src.put(case["x"])
    outs = []
    for _ in range(2):
        d.out.body()[:] = 0x77
        assert d.call(src.ptr, d.L.INGEST_F32, nsamp.data_ptr(), draw=1) == 0, d.err()
        torch.cuda.synchronize()
        outs.append((d.out.get(np.uint8).tobytes(), d.plan.get(np.uint8).tobytes(), d.e_rows().tobytes()))
    assert outs[0] == outs[1] and d.draws() == 0
    steps = []
    for i in range(2):
        assert d.call(src.ptr, d.L.INGEST_F32, nsamp.data_ptr()) == 0, d.err()
        torch.cuda.synchronize()
        steps.append(d.out.get(np.float32).reshape(B, S))
        assert d.plan.get(np.int32).tobytes() == ref["x", i]["plan"].tobytes()
        assert np.array_equal(_bits(steps[i]), _bits(ref["x", i]["out"])) and d.draws() == i + 1
    assert not np.array_equal(_bits(steps[0]), _bits(steps[1])) and d.intact()


def test_a_captured_graph_draws_anew_on_every_replay(rt, case, ref, nsamp):
    d = Dev(rt, case)
    src = Guarded(case["x"].nbytes)
    src.put(case["x"])
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert d.call(src.ptr, d.L.INGEST_F32, nsamp.data_ptr(), stream=C.c_void_p(s.cuda_stream)) == 0, d.err()
    torch.cuda.synchronize()
    assert d.draws() == 0                                        # capture enqueues nothing
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(d.out.get(np.float32).reshape(B, S)), _bits(ref["x", i]["out"])), i
        assert d.plan.get(np.int32).tobytes() == ref["x", i]["plan"].tobytes() and d.draws() == i + 1
    assert d.intact()


def test_a_row_does_not_depend_on_its_batch(rt, case, ref, nsamp):
    mixed = [b for b in range(B) if any(ref["x", dr]["rows"][b]["mixed"] and LENS[b] > 1 for dr in range(3))]
    assert 3 in mixed or mixed
    b = 3 if 3 in mixed else mixed[0]
    draw = next(dr for dr in range(3) if ref["x", dr]["rows"][b]["mixed"])
    d = Dev(rt, case, rows=1)
    src = Guarded(4 * S)
    src.put(case["x"][b])
    n1 = torch.tensor([LENS[b]], dtype=torch.int64, device=DEV)
    assert d.call(src.ptr, d.L.INGEST_F32, n1.data_ptr(), draw=draw, row0=b) == 0, d.err()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d.out.get(np.float32)), _bits(ref["x", draw]["out"][b]))
    assert d.plan.get(np.int32).tobytes() == ref["x", draw]["plan"][b].tobytes()
    assert d.e_rows()[0] == ref["x", draw]["e_rows"][b] and d.intact()


def test_every_refusal_leaves_the_canaries_intact(rt, case, nsamp):
    d = Dev(rt, case)
    L, lib, ctx = d.L, d.lib, d.ctx
    src = Guarded(case["x"].nbytes)
    src.put(case["x"])
    amp = case["amp"]
    firstp = lambda a: np.ascontiguousarray(a, np.int64).ctypes.data_as(C.POINTER(C.c_int64))

    def reset(cfg=None, state=None, nbytes=None, bank=None, first=d.first, n_clips=None, cfgp=True):
        cfg = d.cfg if cfg is None else cfg
        return lib.uvad_mix_reset(ctx, d.state.ptr if state is None else state, d.state.n if nbytes is None else nbytes,
                                  C.byref(cfg) if cfgp else None, d.bank.ptr if bank is None else bank,
                                  None if first is None else firstp(first), d.n_clips if n_clips is None else n_clips, None)

    bad_amp = amp.copy()
    bad_amp[3] = -1.0
    nan_amp = amp.copy()
    nan_amp[0] = np.nan
    null_amp = _cfg(L, amp)
    null_amp.h_amp = None
    resets = [dict(state=0), dict(bank=0), dict(first=None), dict(cfgp=False), dict(state=d.state.ptr + 8), dict(cfg=_cfg(L, amp, mix_prob=-0.1)),
              dict(cfg=_cfg(L, amp, mix_prob=1.5)), dict(cfg=_cfg(L, amp, mix_prob=math.nan)), dict(cfg=_cfg(L, amp, mix_prob=math.inf)),
              dict(cfg=L.MixCfg(0.5, 0, amp.ctypes.data_as(C.POINTER(C.c_double)), 8, 1)), dict(cfg=null_amp), dict(cfg=_cfg(L, bad_amp)),
              dict(cfg=_cfg(L, nan_amp)), dict(cfg=_cfg(L, amp, max_seg=0)), dict(cfg=_cfg(L, amp, max_seg=65)), dict(n_clips=0),
              dict(first=[0, 1, 1, 4, 5, 6, 7]), dict(first=[0, 5, 4, 6, 7, 8, 9]), dict(first=[1, 2, 3, 4, 5, 6, 7]), dict(nbytes=d.state.n - 1)]
    for kw in resets:
        assert reset(**kw) == E_ARG, kw
    assert lib.uvad_mix_reset(None, d.state.ptr, d.state.n, C.byref(d.cfg), d.bank.ptr, firstp(d.first), d.n_clips, None) == E_ARG
    assert lib.uvad_mix_state_bytes(None, 6) == 0 and lib.uvad_mix_state_bytes(C.byref(_cfg(L, amp, max_seg=0)), 6) == 0
    assert lib.uvad_mix_state_bytes(C.byref(d.cfg), 0) == 0 and lib.uvad_mix_ws_bytes(0, 8) == 0 and lib.uvad_mix_ws_bytes(5, 65) == 0

    def step(apply, d_in=src.ptr, fmt=L.INGEST_F32, rows=B, samples=S, out=d.out.ptr, state=d.state.ptr, sbytes=d.state.n, ws=d.ws.ptr,
             wbytes=d.ws.n, plan=d.plan.ptr):
        head = (ctx, d_in, fmt, rows, samples, nsamp.data_ptr(), out, plan)
        tail = (state, sbytes, ws, wbytes, None)
        return lib.uvad_mix_apply(*head, 0, 0, *tail) if apply else lib.uvad_mix_step(*head, *tail)

    never = Guarded(d.state.n)
    for apply in (False, True):
        for kw in (dict(d_in=0), dict(out=0), dict(state=0), dict(ws=0), dict(state=d.state.ptr + 8), dict(ws=d.ws.ptr + 4), dict(fmt=2), dict(fmt=-1),
                   dict(rows=0), dict(samples=0), dict(samples=1 << 31), dict(sbytes=d.state.n - 1), dict(wbytes=d.ws.n - 1), dict(out=d.out.ptr + 2),
                   dict(d_in=src.ptr + 2), dict(fmt=L.INGEST_I16, d_in=d.out.ptr)):
            assert step(apply, **kw) == E_ARG, (apply, kw)
        assert step(apply, state=never.ptr) == E_STATE and "uvad_mix_reset" in d.err()
    torch.cuda.synchronize()
    assert d.intact() and src.intact() and never.intact() and d.draws() == 0
    assert (d.out.get(np.uint8) == 0x77).all() and (d.plan.get(np.uint8) == 0x77).all()


# ---- the host layer ------------------------------------------------------------------------------------------------------------------------
def test_mix_open_and_mix_step(rt, case, ref):
    st = rt.mix_open(case["bank"], CLIPS, snr=(10, 20), mix_prob=0.5, snr_steps=Q, max_seg=MAX_SEG, seed=SEED)
    assert np.array_equal(st["amp"], case["amp"]) and np.array_equal(rt.mix_clip_energies(st), case["e_clips"])
    x = torch.from_numpy(case["x"]).to(DEV)
    out, plan = rt.mix_step(st, x, nsamp=LENS, plan=True)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref["x", 0]["out"])) and plan.cpu().numpy().tobytes() == ref["x", 0]["plan"].tobytes()
    assert np.array_equal(rt.mix_row_energies(st, B), ref["x", 0]["e_rows"])
    q = torch.from_numpy(case["q"]).to(DEV)
    out = rt.mix_step(st, q, nsamp=torch.tensor(LENS, device=DEV))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref["q", 1]["out"])) and rt.mix_draws(st) == 2
    y = x.clone()
    assert rt.mix_step(st, y, nsamp=LENS, out=y, draw=2) is y and rt.mix_draws(st) == 2
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(ref["x", 2]["out"]))
    with pytest.raises(ValueError):
        rt.mix_open(case["bank"], [3, 0, 5])
    with pytest.raises(ValueError):
        rt.mix_open(case["bank"], CLIPS, mix_prob=1.5)
    with pytest.raises(ValueError):
        rt.mix_open(case["bank"][:10], CLIPS)


def _wav(path, x):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
    return str(path)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """Two speech-like recordings with label files, and two noise files."""
    from uvad_amd.synth import synth_pcm
    d = tmp_path_factory.mktemp("mix_corpus")
    paths, labels = [], []
    for k in range(2):
        x = synth_pcm(1, int(1.2 * 16000) + 300 * (1 - k), seed=700 + k)[0]
        x[int(0.3 * 16000):int(0.6 * 16000)] *= 0.02
        paths.append(_wav(d / f"a{k}.wav", x))
        (d / f"a{k}.txt").write_text("0.0\t0.3\tSPC\n0.6\t1.2\tSPC\n")
        labels.append(str(d / f"a{k}.txt"))
    rng = np.random.default_rng(5)
    noise = [_wav(d / "n0.wav", rng.standard_normal(5000) * 0.2), _wav(d / "n1.wav", rng.standard_normal(30000) * 0.05)]
    return {"dir": d, "paths": paths, "labels": labels, "noise": noise}


def _train_cfg(corpus, front, where, noise):
    from config.config import load_config
    cfg = load_config()
    if front == "sincnet":
        cfg.feature_extractor, cfg.model_name, cfg.frame_shift = "sincnet", "PyanNet", 0.02
        cfg.model_dict.encoding_dim = 60
    else:
        cfg.model_dict.encoding_dim = 64
    cfg.model_dict.lstm = {"hidden_size": 64, "num_layers": 1, "dropout": 0.0}
    cfg.model_dict.linear = {"hidden_size": 32, "num_layers": 1}
    cfg.input.kind, cfg.input.paths, cfg.input.labels = "wav", corpus["paths"], corpus["labels"]
    cfg.function, cfg.learning_rate, cfg.max_epochs, cfg.check_val_every_n_epoch = "train", 1e-2, 2, 2
    cfg.window_seconds, cfg.max_duration, cfg.accumulate_grad_batches = 0.4, 0.8, 1
    cfg.experiments_dir = str(corpus["dir"] / where)
    cfg.noise = noise
    return cfg


@pytest.mark.parametrize("front", ["fbank", "sincnet"])
def test_train_vad_with_noise(corpus, front):
    from uvad_amd.scripts import train_vad
    noise = {"paths": corpus["noise"], "snr": (10, 20), "mix_prob": 0.5}
    clean = train_vad(**_train_cfg(corpus, front, front + "_clean", None))
    got = train_vad(**_train_cfg(corpus, front, front + "_noise", noise))
    again = train_vad(**_train_cfg(corpus, front, front + "_again", dict(noise)))
    for run in (clean, got):
        assert len(run["train_loss"]) == 2 and np.isfinite(run["train_loss"]).all() and np.isfinite([l for _, l in run["val_loss"]]).all()
    assert got["train_loss"] != clean["train_loss"]
    assert again["train_loss"] == got["train_loss"] and again["val_loss"] == got["val_loss"]      # one seed: the same draws, the same numbers
    musan = _train_cfg(corpus, front, front + "_musan", None)
    musan.enable_musan, musan.musan = True, {"paths": corpus["noise"], "snr": (10, 20), "mix_prob": 0.5}
    assert train_vad(**musan)["train_loss"] == got["train_loss"]                                   # the reference's keys map to the same run
    if front == "sincnet":
        off = train_vad(**_train_cfg(corpus, front, front + "_off", {"mix_prob": 0}))
        assert off["train_loss"] == clean["train_loss"] and off["val_loss"] == clean["val_loss"]   # the stage runs and changes no bit
    with pytest.raises(ValueError, match="paths"):
        train_vad(**_train_cfg(corpus, front, front + "_bad", {"mix_prob": 0.5}))
