"""The sampler stage on the device (uvad_sampler_*, include/uvad.h) against tests/sampler_ref.py, byte for byte: plan records, gathered rows,
sample counts, labels and frame counts; window edges in both sample formats with output rows 4 bytes off a 16-byte boundary; shuffled epochs,
drop_last, table order; weighted datasets; step / apply / resume; graph replay alone and in front of mix_step and fbank; the refusals
that need a reset state."""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG, E_STATE = -1, -3
SINC = dict(stride=10, n_filters=80, kernel_size=251, c2=60, k2=5, c3=60, k3=5)
W_OF = {"fbank": 1600, "sincnet": 3000}
KEEP = 600
SEED = 0x1234567887654321


@pytest.fixture(scope="module")
def rts():
    from uvad_amd import FbankConfig
    from uvad_amd.runtime import VadRuntime
    model = {"encoding_dim": 60, "lstm": {"hidden_size": 64, "num_layers": 1, "bidirectional": True}, "linear": {"hidden_size": 32, "num_layers": 1},
             "leaky_slope": 0.01}                        # uvad_sincnet_configure wants a model to feed; no weights are loaded
    r = {"fbank": VadRuntime(DEV, fbank=FbankConfig(num_filters=64)), "sincnet": VadRuntime(DEV, model=model, sincnet=SINC)}
    yield r
    for v in r.values():
        v.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _corpus(W, fmt):
    """Seven recordings: tails of exactly min_keep (dropped) and one more (kept), one too short for a window, W, W - 1, W + 1, and 3 W + 37 (an
    odd source offset for everything behind it would need a recording behind it: the odd lengths in front do that for recordings 1 .. 6)."""
    lens = [2 * W + KEEP, 2 * W + KEEP + 1, KEEP - 1, W, W - 1, W + 1, 3 * W + 37]
    rng = np.random.default_rng(11)
    if fmt == "i16":
        pcm = rng.integers(-32768, 32768, sum(lens), dtype=np.int16)
    else:
        pcm = (rng.standard_normal(sum(lens)) * 0.1).astype(np.float32)
        pcm[7], pcm[2 * W + KEEP + 5] = -0.0, np.float32(np.nan)
        pcm.view(np.uint32)[2 * W + KEEP + 9] = 0x7FC12345                       # a NaN payload
    n1 = lens[1]
    sups = [[(10, 200)],
            [(W - 100, W + 100), (2 * W - 1, 2 * W + 1), (2 * W + 300, n1), (0, 50), (-50, 30), (n1 - 100, n1 + 9999), (500, 500), (700, 650),
             (W + 100, W + 400), (W + 300, W + 900), (-(1 << 62), -5), (n1 + 5, 1 << 62)],
            [(0, 100)],
            [],                                                                   # a recording without supervisions
            [(0, W - 1)],
            [(0, W + 1), (W, W + 1)],
            [(int(a), int(a + d)) for a, d in zip(rng.integers(-200, 3 * W + 200, 300), rng.integers(0, 400, 300))]]   # more than one workgroup's threads
    return pcm, lens, sups


def _ref(rt, geometry, pcm, lens, sups, **kw):
    frames = (lambda n: rt.num_frames(n)) if geometry == "fbank" else (lambda n: int(rt.lib.uvad_sincnet_num_frames(rt.ctx, n)))
    sm = S.Sampler(pcm, lens, sups, W_OF[geometry], KEEP, S.FBANK if geometry == "fbank" else S.SINCNET, frames, **kw)
    assert sm.T == (S.frames_fbank if geometry == "fbank" else S.frames_sincnet)(W_OF[geometry])       # the restated counts are the library's
    return sm


def _open(rt, geometry, pcm, lens, sups, **kw):
    return rt.sampler_open(torch.from_numpy(pcm), lens, sups, W_OF[geometry], KEEP, geometry, **kw)


def _host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in res.items()}


def _same(got, want, W, T):
    assert got["plan"].tobytes() == want["plan"].tobytes(), (got["plan"], want["plan"])
    assert np.array_equal(_bits(got["pcm"][:, :W]), _bits(want["out"]))
    assert np.array_equal(got["nsamp"], want["nsamp"]) and np.array_equal(got["frames"], want["frames"])
    assert np.array_equal(got["labels"][:, :T], want["labels"])


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("geometry", ["fbank", "sincnet"])
def test_window_edges_and_labels(rts, geometry, fmt, pad):
    rt, W = rts[geometry], W_OF[geometry]
    pcm, lens, sups = _corpus(W, fmt)
    sm = _ref(rt, geometry, pcm, lens, sups, shuffle=False, pad=bool(pad), seed=SEED)
    assert sm.N[0] == 11 and [tuple(r) for r in sm.windows[:5]] == [(0, 0, W), (0, W, W), (1, 0, W), (1, W, W), (1, 2 * W, KEEP + 1)]
    st = _open(rt, geometry, pcm, lens, sups, shuffle=False, pad=bool(pad), seed=SEED)
    B, T, ld, ldg = 13, sm.T, W + 7, sm.T + 5                                  # more rows than windows: the walk wraps into epoch 1
    flat = torch.full((B * ld + 1,), float("nan"), device=DEV)
    out = flat[1:].view(B, ld)                                                 # rows start 4 bytes off a 16-byte boundary, and 12, 4, 12 ...
    assert out.data_ptr() % 16 == 4
    lab = torch.full((B, ldg), 0xAB, dtype=torch.uint8, device=DEV)
    got = _host(rt.sampler_step(st, B, out=out, labels=lab, plan=True))
    want = sm.step(B)
    _same(got, want, W, T)
    assert np.isnan(got["pcm"][:, W:]).all() and (got["labels"][:, T:] == 0xAB).all() and np.isnan(flat[:1].cpu().numpy()).all()
    assert (want["nsamp"] == W).all() if pad else sorted(set(want["nsamp"])) == [KEEP + 1, W - 1, W]
    assert want["labels"].any() and not want["labels"][want["plan"][:, 4] == 3].any() and want["labels"][want["plan"][:, 4] == 6].any()
    if fmt == "f32":
        assert 0x7FC12345 in _bits(got["pcm"]) and 0x80000000 in _bits(got["pcm"])
    assert rt.sampler_read(st).tolist() == [1, B]


@pytest.mark.parametrize("mode", ["shuffle", "drop_last", "table_order"])
def test_epochs(rts, mode):
    rt, W, B = rts["fbank"], W_OF["fbank"], 4
    pcm, lens, sups = _corpus(W, "f32")
    kw = dict(shuffle=mode != "table_order", drop_last=mode == "drop_last", batch=B, seed=SEED)
    sm, st = _ref(rt, "fbank", pcm, lens, sups, **kw), _open(rt, "fbank", pcm, lens, sups, **kw)
    L = 8 if mode == "drop_last" else 11
    assert sm.N[0] == 11 and sm.L[0] == L
    plans = []
    for _ in range(9):                                                         # 36 rows: three whole epochs, B not dividing N
        got, want = _host(rt.sampler_step(st, B, plan=True)), sm.step(B)
        _same(got, want, W, sm.T)
        plans.append(got["plan"])
    plan = np.concatenate(plans)
    for e in range(3):
        rows = plan[plan[:, 1] == e]
        assert len(rows) == L and len(set(rows[:, 3])) == L and np.array_equal(rows[:, 2], np.arange(L))
        if mode == "table_order":
            assert np.array_equal(rows[:, 3], np.arange(11))
    if mode == "shuffle":
        orders = [plan[plan[:, 1] == e][:, 3].tolist() for e in range(3)]
        assert orders[0] != orders[1] != orders[2] and orders[0] != list(range(11))
    assert rt.sampler_read(st).tolist() == [9, 36]


def test_weighted_datasets(rts):
    rt, W, B = rts["fbank"], W_OF["fbank"], 4
    lens, sets, weights = [3 * W, 5 * W, 4 * W, 5 * W], [0, 1, 2, 2], (1.0, 2.0, 5.0)          # N_d = 3, 5, 9
    pcm = (np.random.default_rng(3).standard_normal(sum(lens)) * 0.1).astype(np.float32)
    sups = [[(100, 900)], [], [(W, 2 * W)], []]
    sm = _ref(rt, "fbank", pcm, lens, sups, rec_set=sets, weights=weights, seed=SEED)
    st = _open(rt, "fbank", pcm, lens, sups, datasets=sets, weights=weights, seed=SEED)
    assert sm.N.tolist() == [3, 5, 9]
    seen = np.zeros(3, np.int64)
    for i in range(40):
        got, want = _host(rt.sampler_step(st, B, plan=True)), sm.step(B)
        _same(got, want, W, sm.T)
        seen += np.bincount(got["plan"][:, 0], minlength=3)
    assert rt.sampler_read(st).tolist() == [40] + sm.cursor.tolist() and sm.cursor.tolist() == seen.tolist()
    assert seen[0] >= 3 * 3 and seen[2] > seen[1] > seen[0]                    # the smallest dataset wrapped several times


def test_step_apply_and_resume(rts):
    rt, W, B = rts["sincnet"], W_OF["sincnet"], 5
    lens, sets, weights = [3 * W + 700, 2 * W, 4 * W + 1], [0, 1, 1], (1.0, 3.0)
    pcm = np.random.default_rng(5).integers(-32768, 32768, sum(lens), dtype=np.int16)
    sups = [[(0, 2000), (W, 2 * W + 5)], [(50, 60)], [(W - 10, 3 * W)]]
    kw = dict(datasets=sets, weights=weights, seed=SEED, pad=True)
    st = _open(rt, "sincnet", pcm, lens, sups, **kw)
    for _ in range(3):
        rt.sampler_step(st, B)
    rec = rt.sampler_read(st)
    assert rec[0] == 3 and rec[1:].sum() == 15
    stepped = _host(rt.sampler_step(st, B, plan=True))
    after = rt.sampler_read(st)
    applied = _host(rt.sampler_step(st, B, plan=True, cursor=rec[1:], draw=int(rec[0])))
    assert all(stepped[k].tobytes() == applied[k].tobytes() for k in stepped)
    assert rt.sampler_read(st).tolist() == after.tolist()                      # apply updated nothing
    rank = np.zeros(2, np.int64)
    for b in range(B):                                                         # row b alone, under its own index and cursor
        d = int(stepped["plan"][b, 0])
        cur = rec[1:].copy()
        cur[d] += rank[d]
        rank[d] += 1
        one = _host(rt.sampler_step(st, 1, plan=True, cursor=cur, draw=int(rec[0]), row0=b))
        assert all(one[k][0].tobytes() == stepped[k][b].tobytes() for k in stepped), b
    fresh = _open(rt, "sincnet", pcm, lens, sups, **kw)
    rt.sampler_write(fresh, rec)
    assert rt.sampler_read(fresh).tolist() == rec.tolist()
    again = _host(rt.sampler_step(fresh, B, plan=True))
    assert all(stepped[k].tobytes() == again[k].tobytes() for k in stepped)
    for _ in range(2):
        a, b = _host(rt.sampler_step(st, B, plan=True)), _host(rt.sampler_step(fresh, B, plan=True))
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_a_captured_graph_draws_a_new_batch_on_every_replay(rts):
    rt, W, B = rts["fbank"], W_OF["fbank"], 4
    pcm, lens, sups = _corpus(W, "f32")
    st, twin = _open(rt, "fbank", pcm, lens, sups, seed=SEED), _open(rt, "fbank", pcm, lens, sups, seed=SEED)
    rt.sampler_step(st, B, plan=True, cursor=[0], draw=0)                      # the buffers of this batch size; no state update
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            res = rt.sampler_step(st, B, plan=True)
    torch.cuda.synchronize()
    assert rt.sampler_read(st).tolist() == [0, 0]                              # capture enqueues nothing
    seen = []
    for i in range(3):
        g.replay()
        got, want = _host(res), _host(rt.sampler_step(twin, B, plan=True))
        assert all(got[k].tobytes() == want[k].tobytes() for k in got), i
        seen.append(got["plan"][:, 3].tolist())
    assert seen[0] != seen[1] and rt.sampler_read(st).tolist() == [3, 12]


def test_one_graph_of_sampler_mix_and_fbank(rts):
    rt, W, B = rts["fbank"], W_OF["fbank"], 4
    pcm, lens, sups = _corpus(W, "f32")
    noise = (np.random.default_rng(9).standard_normal(5000) * 0.05).astype(np.float32)

    def chain(st, mx, mixed):
        res = rt.sampler_step(st, B, plan=True)
        rt.mix_step(mx, res["pcm"], nsamp=res["nsamp"], out=mixed)
        return res, rt.fbank(mixed, lengths=res["nsamp"])

    def make():
        return (_open(rt, "fbank", pcm, lens, sups, seed=SEED), rt.mix_open(torch.from_numpy(noise), [2000, 3000], mix_prob=1.0, seed=SEED),
                torch.zeros((B, W), device=DEV))
    a, b = make(), make()
    rt.sampler_step(a[0], B, plan=True, cursor=[0], draw=0)                    # allocate the buffers outside the capture
    rt.mix_step(a[1], torch.zeros((B, W), device=DEV), nsamp=torch.full((B,), W, dtype=torch.int64, device=DEV), out=a[2], draw=0)
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            res, feats = chain(*a)
    torch.cuda.synchronize()
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        want_res, want_feats = chain(*b)
        torch.cuda.synchronize()
        assert all(res[k].cpu().numpy().tobytes() == want_res[k].cpu().numpy().tobytes() for k in res), i
        assert a[2].cpu().numpy().tobytes() == b[2].cpu().numpy().tobytes() and feats.cpu().numpy().tobytes() == want_feats.cpu().numpy().tobytes(), i
        assert not np.array_equal(a[2].cpu().numpy(), res["pcm"].cpu().numpy())            # noise went in


def test_refusals_of_a_reset_state_leave_the_outputs_alone(rts):
    rt, W, B = rts["fbank"], W_OF["fbank"], 4
    pcm, lens, sups = _corpus(W, "f32")
    st = _open(rt, "fbank", pcm, lens, sups, seed=SEED, drop_last=True, batch=B)
    lib, T = rt.lib, st["T"]
    out = torch.full((B + 1, W), 7.0, device=DEV)
    lab = torch.full((B + 1, T), 0xAB, dtype=torch.uint8, device=DEV)
    ns, fr = torch.full((B + 1,), -1, dtype=torch.int64, device=DEV), torch.full((B + 1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(int(lib.uvad_sampler_ws_bytes(B + 1)), dtype=torch.uint8, device=DEV)
    err = lambda: lib.uvad_last_error(rt.ctx).decode()

    def step(apply=False, B=B, ld_out=W, ld_gt=T, nbytes=st["state"].numel(), ws_bytes=ws.numel(), cur=(0,), ctx=rt):
        head = (ctx.ctx, B, out.data_ptr(), ld_out, ns.data_ptr(), lab.data_ptr(), ld_gt, fr.data_ptr(), None)
        tail = (st["state"].data_ptr(), nbytes, ws.data_ptr(), ws_bytes, None)
        return lib.uvad_sampler_apply(*head, (C.c_int64 * 1)(*cur), 0, 0, *tail) if apply else lib.uvad_sampler_step(*head, *tail)
    for apply in (False, True):
        assert step(apply, ld_out=W - 1) == E_ARG and "ld_out" in err()
        assert step(apply, ld_gt=T - 1) == E_ARG and "ld_gt" in err()
        assert step(apply, B=B + 1) == E_ARG and "drop_last" in err() and step(apply, B=B - 1) == E_ARG
        assert step(apply, nbytes=st["state"].numel() - 1) == E_ARG and "state too small" in err()
        assert step(apply, ws_bytes=int(lib.uvad_sampler_ws_bytes(B)) - 1) == E_ARG and "workspace too small" in err()
    assert step(True, cur=(-1,)) == E_ARG and "cursor" in err()
    from uvad_amd.runtime import VadRuntime
    other = VadRuntime(DEV)                      # a context that never reset a state (one that did may still know this address from a freed one)
    try:
        assert step(ctx=other) == E_STATE and "uvad_sampler_reset" in lib.uvad_last_error(other.ctx).decode()
    finally:
        other.close()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (lab == 0xAB).all() and (ns == -1).all() and (fr == -1).all() and rt.sampler_read(st).tolist() == [0, 0]
    assert step() == 0 and step(True) == 0, err()
    torch.cuda.synchronize()
    assert (out[B] == 7.0).all() and (lab[B] == 0xAB).all() and ns[B] == -1 and fr[B] == -1 and (ns[:B] > 0).all()
    with pytest.raises(Exception, match="without windows"):
        rt.sampler_open(torch.from_numpy(pcm[:KEEP]), [KEEP], [[]], W, KEEP, "fbank")
    with pytest.raises(Exception, match="gives no frame"):
        rts["sincnet"].sampler_open(torch.from_numpy(pcm[:900]), [900], [[]], 700, 0, "sincnet")


def _wav(path, x):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
    return str(path)


@pytest.fixture(scope="module")
def wav_corpus(tmp_path_factory):
    """Three speech-like recordings of different lengths with label files, in two datasets."""
    from uvad_amd.synth import synth_pcm
    d = tmp_path_factory.mktemp("sampler_corpus")
    paths, labels = [], []
    for k, seconds in enumerate((1.3, 0.9, 1.65)):
        x = synth_pcm(1, int(seconds * 16000) + 37 * k, seed=800 + k)[0]
        x[int(0.3 * 16000):int(0.6 * 16000)] *= 0.02
        paths.append(_wav(d / f"a{k}.wav", x))
        (d / f"a{k}.txt").write_text(f"0.0\t0.3\tSPC\n0.6\t{seconds}\tSPC\n")
        labels.append(str(d / f"a{k}.txt"))
    return {"dir": d, "paths": paths, "labels": labels, "datasets": ["x", "y", "x"]}


def _train_cfg(corpus, front, where, **kw):
    from config.config import load_config
    cfg = load_config()
    if front == "sincnet":
        cfg.feature_extractor, cfg.model_name, cfg.frame_shift = "sincnet", "PyanNet", 0.02
        cfg.model_dict.encoding_dim = 60
    else:
        cfg.model_dict.encoding_dim = 64
    cfg.model_dict.lstm = {"hidden_size": 64, "num_layers": 1, "dropout": 0.0}
    cfg.model_dict.linear = {"hidden_size": 32, "num_layers": 1}
    cfg.input.kind, cfg.input.paths, cfg.input.labels, cfg.input.datasets = "wav", corpus["paths"], corpus["labels"], corpus["datasets"]
    cfg.function, cfg.learning_rate, cfg.max_epochs, cfg.check_val_every_n_epoch = "train", 1e-2, 2, 2
    cfg.window_seconds, cfg.max_duration, cfg.accumulate_grad_batches = 0.4, 0.8, 1
    cfg.experiments_dir = str(corpus["dir"] / where)
    cfg.device_sampler, cfg.dataset_weights = True, {"x": 1.0, "y": 3.0}
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("front", ["fbank", "sincnet"])
def test_train_vad_with_the_device_sampler(wav_corpus, front):
    from uvad_amd.scripts import sampler_corpus, train_vad
    whole = train_vad(**_train_cfg(wav_corpus, front, front + "_whole"))
    assert len(whole["train_loss"]) == 2 and np.isfinite(whole["train_loss"]).all() and np.isfinite([l for _, l in whole["val_loss"]]).all()
    blob = torch.load(whole["checkpoint_path"], map_location="cpu", weights_only=True)
    spe, rows = whole["steps_per_epoch"], 2
    assert blob["epoch"] == 2 and blob["global_step"] == 2 * spe and blob["optimizer_states"]["sampler"][0] == 2 * spe
    assert sum(blob["optimizer_states"]["sampler"][1:]) == 2 * spe * rows
    # the first batch is the sampler's at cursor 0 and draw 0
    from uvad_amd import FbankConfig
    from uvad_amd.runtime import VadRuntime
    model = {"encoding_dim": 60, "lstm": {"hidden_size": 64, "num_layers": 1, "bidirectional": True}, "linear": {"hidden_size": 32, "num_layers": 1}}
    rt = VadRuntime(DEV, fbank=FbankConfig(num_filters=64)) if front == "fbank" else VadRuntime(DEV, model=model, sincnet=SINC)
    try:
        pcm, lens, sups = sampler_corpus(wav_corpus["paths"], wav_corpus["labels"], rt)
        keep = 79 if front == "fbank" else int(round(0.6 * 0.4 * 16000))
        sm = S.Sampler(pcm, lens, sups, 6400, keep, S.FBANK if front == "fbank" else S.SINCNET,
                       S.frames_fbank if front == "fbank" else S.frames_sincnet, rec_set=[0, 1, 0], weights=(1.0, 3.0), pad=front == "sincnet", seed=42)
        assert spe == sm.N.sum() // rows
        seed = int(_train_cfg(wav_corpus, front, "x").seed)
        sm.seed = seed
        assert whole["first_plan"].tobytes() == sm.apply(rows, [0, 0], 0)["plan"].tobytes()
    finally:
        rt.close()
    # interrupted after epoch 1 and resumed: the uninterrupted run's checkpoint bytes
    part = train_vad(**_train_cfg(wav_corpus, front, front + "_part", stop_after_epoch=1))
    rest = train_vad(**_train_cfg(wav_corpus, front, front + "_rest", load_checkpoint=True, checkpoint_path=part["checkpoint_path"]))
    got = torch.load(rest["checkpoint_path"], map_location="cpu", weights_only=True)
    assert got["optimizer_states"]["sampler"] == blob["optimizer_states"]["sampler"] and got["global_step"] == blob["global_step"]
    for k, v in blob["state_dict"].items():
        assert v.numpy().tobytes() == got["state_dict"][k].numpy().tobytes(), k
    assert rest["train_loss"] == whole["train_loss"][1:] and rest["val_loss"] == whole["val_loss"]
    # the default stays the host path
    host = train_vad(**_train_cfg(wav_corpus, front, front + "_host", device_sampler=False))
    assert host.get("first_plan") is None and len(host["train_loss"]) == 2 and host["train_loss"] != whole["train_loss"]
