"""The joint optimizer step on the device (uvad_optim_step and the _write calls, include/uvad.h) against tests/optim_ref.py, bit for bit.
Chains, the smallest that still have several reduction chunks and a ragged tail:
  "lstm"     PyanNet2, hidden 64, bidirectional, 2 layers on 80 features, head 32 / 1, B 3, T 19, lengths (19, 7, 1): head P = 4161 (two
             chunks, the second ragged), LSTM P = 174080 (42.5 chunks)
  "sincnet"  PyanNet (one bidirectional 64-unit layer, head 32 / 1), B 2, S 991 (one frame): all three families
  "head0"    a head without feed-forward layers on D0 = 64: P = 65, less than a chunk
A family of more than 256 chunks, whose partials opt_fold_kernel takes through LDS in a second pass (256, 257 and the reference model's 342),
lives in tests/test_gpu_train_reference_size.py, which builds its chains here through Chain's shape arguments.
Cases: off is off, clipping, weight decay, the table and lr_scale, absent and idle states, a non-finite step, a captured graph, the device
guards, the read / write round trip into a fresh context, and train_vad with every option and a resumed run."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R
import sincnet_train_ref as SR
import test_gpu_head_train as T1
import test_gpu_lstm_train as T0
import test_gpu_sincnet_train as T2

gpu = pytest.mark.gpu
PAD, CANARY = 256, 0xA5
F32 = np.float32


def _dev():
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def _flat(d):
    return np.concatenate([t.numpy().reshape(-1) for t in d.values()])


class Chain:
    """One of the three chains on a fresh runtime: handles, seeded batches, forward / backward, and either kind of step."""

    def __init__(self, kind, dropout=0.0, lr=1e-3, rt=None, Din=80, H=64, layers=2, B=3, T=19, lens=(19, 7, 1)):
        """Din, H, layers, B, T, lens: the "lstm" chain's model and batch (the defaults are the chain of the module's docstring)."""
        self.kind, self.hl, self.hs, self.lens, self.Din = kind, None, None, None, Din if kind == "lstm" else 64
        if kind == "lstm":
            self.rt = rt or T0._runtime(Din, H, 2, layers)[0]
            self.hh = self.rt.head_train_open(lr=lr, segment=32)
            self.hl = self.rt.lstm_train_open(layers=layers, lr=lr, segment=32, dropout=dropout, seed=11)
            self.B, self.T, self.lens = B, T, torch.tensor(list(lens), dtype=torch.int32, device=_dev())
        elif kind == "sincnet":
            self.rt = rt or T2._model(SR.make_case(2, 991, 1)[0]).runtime(_dev())
            self.hh = self.rt.head_train_open(lr=lr, segment=32)
            self.hl = self.rt.lstm_train_open(layers=1, lr=lr, segment=32)
            self.hs = self.rt.sincnet_train_open(first_stage=0, lr=lr, segment=32)
            self.B, self.T = 2, SR.num_frames(991)
        else:
            self.rt = rt or T1._head_runtime(64, 32, 0, 0.01)[0]
            self.hh = self.rt.head_train_open(lr=lr, segment=32)
            self.B, self.T, self.lens = 3, 19, torch.tensor([19, 7, 1], dtype=torch.int32, device=_dev())
        self.handles = (self.hh, self.hl, self.hs)
        self.buf = None

    def batch(self, k):
        rng = np.random.default_rng(5000 + k)
        gt = torch.from_numpy((rng.random((self.B, self.T)) < 0.5).astype(np.uint8)).to(_dev())
        if self.kind == "sincnet":
            x = torch.from_numpy(SR.make_case(self.B, 991, 70 + k)[1].astype(F32)).to(_dev())
        else:
            x = torch.from_numpy(rng.standard_normal((self.B, self.T, self.Din)).astype(F32)).to(_dev())
        return x, gt

    def fb(self, k=None, dz=None, data=None):
        """Forward and backward of batch k (or of the tensors given): the gradients land in the accumulators, no step."""
        x, gt = data if data is not None else self.batch(k)
        rt, feats = self.rt, None
        if self.hs is not None:
            feats = rt.sincnet_train_forward(self.hs, x)
        y = x if self.hl is None else rt.lstm_train_forward(self.hl, feats if feats is not None else x, lengths=self.lens)
        _, gx = rt.head_train_grad(self.hh, y, None if dz is not None else gt, lengths=self.lens, dz=dz, want_grad_x=self.hl is not None)
        if self.hl is not None:
            gin = rt.lstm_train_backward(self.hl, feats if feats is not None else x, gx, lengths=self.lens, want_grad_in=self.hs is not None)
            if self.hs is not None:
                rt.sincnet_train_backward(self.hs, x, gin)

    def apply(self):
        self.rt.head_train_apply(self.hh)
        if self.hl is not None:
            self.rt.lstm_train_apply(self.hl)
        if self.hs is not None:
            self.rt.sincnet_train_apply(self.hs)

    def optim(self, o, **which):
        self.rt.optim_step(o, **(which or dict(head=self.hh, lstm=self.hl, sincnet=self.hs)))

    def reads(self):
        rt = self.rt
        return (rt.head_train_read(self.hh), None if self.hl is None else rt.lstm_train_read(self.hl),
                None if self.hs is None else rt.sincnet_train_read(self.hs))

    def snap(self):
        out = []
        for r in self.reads():
            out.append(None if r is None else {"w": _flat(r["weights"]), "g": _flat(r["grad"]), "m": _flat(r["m"]), "v": _flat(r["v"]),
                                               "frames": r["frames"], "t": r["step"], "bc1": F32(r["bias_correction1"]),
                                               "bc2": F32(r["bias_correction2"]), "loss": r.get("loss", 0.0)})
        return out

    def state_bytes(self):
        torch.cuda.synchronize()
        return tuple(None if h is None else bytes(h["state"].cpu().numpy()) for h in self.handles)

    def optim_open(self, cfg=None, table=(1e-3,), canaries=False):
        """An optimizer handle; canaries: its state and workspace sit inside buffers of CANARY bytes (self.buf), the runtime's wrappers
        then run on views of them."""
        rt = self.rt
        if not canaries:
            return rt.optim_open(cfg, table)
        o = rt.optim_open(cfg, table)
        for h, conf in ((self.hh, rt.lib.uvad_head_train_configure), (self.hs, rt.lib.uvad_sincnet_train_configure)):
            if h is not None:
                rt._check(conf(rt.ctx, C.byref(h["cfg"])))
        if self.hl is not None:
            rt._lstm_train_configure(self.hl)
        ns, nw = int(rt.lib.uvad_optim_state_bytes(o["n"])), int(rt.lib.uvad_optim_ws_bytes(rt.ctx))
        self.buf = torch.full((ns + nw + 3 * PAD,), CANARY, dtype=torch.uint8, device=_dev())
        o["state"], o["ws"] = self.buf[PAD:PAD + ns], self.buf[2 * PAD + ns:2 * PAD + ns + nw]
        rt._check(rt.lib.uvad_optim_reset(rt.ctx, o["state"].data_ptr(), ns, C.byref(o["cfg"]), o["table"].ctypes.data_as(C.POINTER(C.c_float)),
                                          o["n"], None))
        self.spans = ((0, PAD), (PAD + ns, 2 * PAD + ns), (2 * PAD + ns + nw, 3 * PAD + ns + nw))
        return o

    def canaries_intact(self):
        torch.cuda.synchronize()
        return all(bool((self.buf[a:b] == CANARY).all()) for a, b in self.spans)


def _rcfg(cfg):
    cfg = cfg or {}
    return R.default_cfg(max_norm=cfg.get("max_norm", 0.0), weight_decay=cfg.get("weight_decay", 0.0), decoupled=cfg.get("adamw", False),
                         skip_nonfinite=cfg.get("skip_nonfinite", False), lr_scale=cfg.get("lr_scale", (1.0, 1.0, 1.0)))


def _ref_of(snaps):
    return [None if s is None else {"w": s["w"], "m": s["m"], "v": s["v"], "t": s["t"], "bc1": s["bc1"], "bc2": s["bc2"]} for s in snaps]


def _checked_step(ch, o, ref, ropt, cfg, table, k, dz=None):
    """Batch k's gradients, the restatement of the step from the accumulators as read, the device step, and everything compared bit for bit
    -> (families, counts, record) of the restatement."""
    ch.fb(k, dz=dz)
    snaps = ch.snap()
    assert all(s is None or (s["frames"] > 0 and np.abs(s["g"]).max() > 0) for s in snaps)
    want, ropt, rec = R.step([None if s is None else (f, s["g"], s["frames"]) for f, s in zip(ref, snaps)], ropt, _rcfg(cfg), np.asarray(table, F32))
    ch.optim(o)
    got, after = ch.rt.optim_read(o), ch.snap()
    assert (_bits(got["norm"]), _bits(got["coef"]), _bits(got["lr"])) == (_bits(rec["norm"]), _bits(rec["coef"]), _bits(rec["lr"])), (k, got, rec)
    assert sum(1 << i for i, p in enumerate(got["took_part"]) if p) == rec["mask"] and (got["step"], got["skipped"]) == (ropt["t"], ropt["skipped"])
    for i, (a, w) in enumerate(zip(after, want)):
        if a is None:
            continue
        for key in ("w", "m", "v", "bc1", "bc2"):
            assert np.array_equal(_bits(a[key]), _bits(w[key])), (k, i, key)
        assert a["t"] == w["t"] and a["frames"] == 0 and a["loss"] == 0.0 and not a["g"].any(), (k, i)
    return want, ropt, rec


def _checked_run(kind, cfg, table, steps, dropout=0.0):
    ch = Chain(kind, dropout=dropout)
    o = ch.optim_open(cfg, table)
    ref, ropt, recs = _ref_of(ch.snap()), {"t": 0, "skipped": 0}, []
    for k in range(steps):
        ref, ropt, rec = _checked_step(ch, o, ref, ropt, cfg, table, k)
        recs.append(rec)
    return ch, o, recs


# ------------------------------------------------------------------------------------------------ 1. off is off
@gpu
@pytest.mark.parametrize("kind", ["lstm", "sincnet", "head0"])
def test_with_every_option_off_the_step_leaves_the_bytes_of_the_apply_calls(kind):
    a, b = Chain(kind), Chain(kind)
    o = b.optim_open({}, [1e-3])                          # max_norm 0, weight_decay 0, lr_scale 1, a one-entry table holding the families' lr
    assert a.state_bytes() == b.state_bytes()
    for k in range(3):
        a.fb(k), a.apply()
        b.fb(k), b.optim(o)
    assert a.state_bytes() == b.state_bytes()             # masters, m, v, scalars: the whole state
    rec = b.rt.optim_read(o)
    assert rec["step"] == 3 and rec["skipped"] == 0 and rec["coef"] == 1.0 and rec["norm"] > 0 and _bits(rec["lr"]) == _bits(F32(1e-3))
    assert rec["took_part"] == tuple(h is not None for h in b.handles) and all(r is None or r["step"] == 3 for r in b.reads())
    a.fb(3), a.optim(a.optim_open({}, [1e-3]))           # mixing apply and the joint step on one state stays well defined
    b.fb(3), b.apply()
    assert a.state_bytes() == b.state_bytes()
    a.rt.close(), b.rt.close()


# ------------------------------------------------------------------------------------------------ 2. clipping
@gpu
@pytest.mark.parametrize("kind", ["lstm", "sincnet", "head0"])
def test_clipping_equals_the_restatement_bit_for_bit_over_seven_steps(kind):
    free, _, recs = _checked_run(kind, {}, [1e-3], 7)
    first = float(recs[0]["norm"])
    assert first > 0 and all(r["coef"] == 1.0 for r in recs)
    tight, _, recs = _checked_run(kind, {"max_norm": 0.5 * first}, [1e-3], 7)          # below the first step's measured norm
    assert recs[0]["coef"] < 1.0 and _bits(recs[0]["norm"]) == _bits(F32(first))
    assert tight.state_bytes() != free.state_bytes()
    loose, _, recs = _checked_run(kind, {"max_norm": 1e6 * first}, [1e-3], 7)          # far above: nothing is clipped
    assert all(r["coef"] == 1.0 for r in recs) and loose.state_bytes() == free.state_bytes()
    for c in (free, tight, loose):
        c.rt.close()


# ------------------------------------------------------------------------------------------------ 3. weight decay
@gpu
def test_weight_decay_in_both_modes_equals_the_restatement_and_moves_the_masters():
    plain, _, _ = _checked_run("lstm", {}, [1e-3], 5)
    base = plain.snap()
    for adamw in (False, True):
        ch, _, _ = _checked_run("lstm", {"weight_decay": 1e-2, "adamw": adamw, "max_norm": 1.0}, [1e-3], 5)
        for a, b in zip(ch.snap(), base):
            assert a is None or not np.array_equal(_bits(a["w"]), _bits(b["w"])), adamw
        ch.rt.close()
    plain.rt.close()


# ------------------------------------------------------------------------------------------------ 4. the table
@gpu
def test_the_table_is_indexed_by_the_applied_steps_and_lr_scale_holds_a_family_still():
    table = [1e-3, 2e-3, 5e-4, 2.5e-4]
    cfg = {"lr_scale": (1.0, 0.1, 0.0)}
    ch = Chain("sincnet")
    o = ch.optim_open(cfg, table)
    start = ch.snap()
    ref, ropt = _ref_of(start), {"t": 0, "skipped": 0}
    for k in range(6):
        ref, ropt, rec = _checked_step(ch, o, ref, ropt, cfg, table, k)
        assert _bits(rec["lr"]) == _bits(F32(table[min(k, 3)]))
    end = ch.snap()
    assert np.array_equal(_bits(end[2]["w"]), _bits(start[2]["w"])) and end[2]["m"].any() and end[2]["v"].any() and end[2]["t"] == 6
    assert not np.array_equal(_bits(end[0]["w"]), _bits(start[0]["w"])) and not np.array_equal(_bits(end[1]["w"]), _bits(start[1]["w"]))
    ch.rt.close()


@gpu
def test_a_table_rewritten_between_replays_of_one_graph_takes_effect_without_capturing_again():
    first, second = [1e-3, 2e-3, 3e-3, 4e-3], [7e-4, 6e-4, 5e-4]
    e, g = Chain("lstm"), Chain("lstm")
    oe, og = e.optim_open({}, first), g.optim_open({}, first)
    for k in range(4):
        if k == 2:
            e.rt.optim_set_lr(oe, second)
        e.fb(k), e.optim(oe)
    sx, sgt = (torch.zeros_like(t) for t in g.batch(0))
    g.fb(data=(sx, sgt))                                  # sizes the workspaces, which the captured handles take over
    fresh = Chain("lstm", rt=g.rt)
    fresh.hh["ws"], fresh.hl["ws"] = g.hh["ws"], g.hl["ws"]
    fresh.optim(og)                                       # no participant: writes nothing, sizes the optimizer's workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fresh.fb(data=(sx, sgt)), fresh.optim(og)
    lrs = []
    for k in range(4):
        if k == 2:
            g.rt.optim_set_lr(og, second)
        x, gt = g.batch(k)
        sx.copy_(x), sgt.copy_(gt)
        graph.replay()
        lrs.append(g.rt.optim_read(og)["lr"])
    assert [_bits(v) for v in lrs] == [_bits(F32(v)) for v in (first[0], first[1], second[2], second[2])]
    assert fresh.state_bytes() == e.state_bytes() and bytes(og["state"].cpu().numpy()) == bytes(oe["state"].cpu().numpy())
    e.rt.close(), g.rt.close()


# ------------------------------------------------------------------------------------------------ 5. absent and idle states
@gpu
def test_an_absent_or_idle_lstm_state_leaves_the_head_stepping_as_alone():
    cfg = {"max_norm": 1e-3, "weight_decay": 1e-2}
    runs = []
    for mode in ("absent", "idle"):
        ch = Chain("lstm")
        o = ch.optim_open(cfg, [1e-3])
        x, gt = ch.batch(0)
        y = ch.rt.lstm_train_forward(ch.hl, x, lengths=ch.lens)                    # forward only: the LSTM state accumulates nothing
        ch.rt.head_train_grad(ch.hh, y, gt, lengths=ch.lens)
        idle = ch.state_bytes()[1]
        s = ch.snap()[0]
        want, _, rec = R.step([(_ref_of([s])[0], s["g"], s["frames"]), None, None], {"t": 0, "skipped": 0}, _rcfg(cfg), np.asarray([1e-3], F32))
        ch.optim(o, head=ch.hh, lstm=None if mode == "absent" else ch.hl)
        got, after = ch.rt.optim_read(o), ch.snap()
        assert _bits(got["norm"]) == _bits(rec["norm"]) and _bits(got["coef"]) == _bits(rec["coef"]), (got, rec)      # the norm is the head's
        assert got["coef"] < 1.0 and got["took_part"] == (True, False, False) and got["step"] == 1, got
        for key in ("w", "m", "v"):
            assert np.array_equal(_bits(after[0][key]), _bits(want[0][key])), (mode, key)
        assert ch.state_bytes()[1] == idle and after[1]["t"] == 0                  # the idle state's bytes are untouched
        runs.append(ch.state_bytes()[0])
        ch.rt.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------ 6. a non-finite step
@gpu
def test_a_non_finite_step_is_skipped_and_the_next_clean_step_equals_the_restatement():
    cfg = {"skip_nonfinite": True, "max_norm": 1.0}
    ch = Chain("lstm")
    o = ch.optim_open(cfg, [1e-3, 2e-3, 3e-3])
    ref, ropt = _ref_of(ch.snap()), {"t": 0, "skipped": 0}
    ref, ropt, _ = _checked_step(ch, o, ref, ropt, cfg, [1e-3, 2e-3, 3e-3], 0)
    before = ch.snap()
    dz = torch.from_numpy(np.random.default_rng(9).standard_normal((ch.B, ch.T)).astype(F32) * 0.1)
    dz[1, 3] = float("nan")                               # a valid frame: row 1 has 7
    ch.fb(1, dz=dz.to(_dev()))
    mid = ch.snap()
    assert all(np.isnan(s["g"]).any() and s["frames"] > 0 for s in mid[:2])
    ch.optim(o)
    got, after = ch.rt.optim_read(o), ch.snap()
    assert got["skipped"] == 1 and got["step"] == 1 and got["coef"] == 0.0 and np.isnan(got["norm"]) and got["took_part"] == (True, True, False)
    for a, b in zip(after[:2], before[:2]):
        for key in ("w", "m", "v", "bc1", "bc2"):
            assert np.array_equal(_bits(a[key]), _bits(b[key])), key
        assert a["t"] == b["t"] == 1 and a["frames"] == 0 and a["loss"] == 0.0 and not a["g"].any()
    ref, ropt = _ref_of(after), {"t": 1, "skipped": 1}
    _, ropt, rec = _checked_step(ch, o, ref, ropt, cfg, [1e-3, 2e-3, 3e-3], 2)      # the next clean step: lr entry 1, not 2
    assert ropt == {"t": 2, "skipped": 1} and _bits(rec["lr"]) == _bits(F32(2e-3))
    ch.rt.close()
    run = Chain("lstm")                                   # skip_nonfinite = 0: the step runs
    o = run.optim_open({}, [1e-3])
    run.fb(1, dz=dz.to(_dev())), run.optim(o)
    assert run.rt.optim_read(o)["step"] == 1 and run.rt.optim_read(o)["skipped"] == 0 and all(s["t"] == 1 for s in run.snap()[:2])
    run.rt.close()


# ------------------------------------------------------------------------------------------------ 7. a captured graph
@gpu
def test_a_captured_step_ending_in_the_joint_step_replays_to_the_eager_bytes():
    table = [1e-3, 2e-3, 3e-3, 2e-3, 1e-3]
    cfg = {"max_norm": 0.5, "weight_decay": 1e-2, "adamw": True, "skip_nonfinite": True}
    e = Chain("lstm", dropout=0.5)
    oe = e.optim_open(cfg, table)
    for k in range(5):
        e.fb(k), e.optim(oe)
    warm = Chain("lstm", dropout=0.5)
    sx, sgt = (torch.zeros_like(t) for t in warm.batch(0))
    warm.fb(data=(sx, sgt))                               # sizes the workspaces, which the captured handles take over
    g = Chain("lstm", dropout=0.5, rt=warm.rt)
    g.hh["ws"], g.hl["ws"] = warm.hh["ws"], warm.hl["ws"]
    og = g.optim_open(cfg, table, canaries=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # one stream; a synchronisation or an allocation of the library's would fail here
        g.fb(data=(sx, sgt)), g.optim(og)
    assert g.rt.optim_read(og)["step"] == 0               # captured, not run
    for k in range(5):
        x, gt = g.batch(k)
        sx.copy_(x), sgt.copy_(gt)
        graph.replay()
    assert g.state_bytes() == e.state_bytes() and g.rt.lstm_train_draws(g.hl) == 5
    assert bytes(og["state"].cpu().numpy()) == bytes(oe["state"].cpu().numpy()) and g.rt.optim_read(og)["step"] == 5
    assert g.canaries_intact()
    e.rt.close(), g.rt.close()


# ------------------------------------------------------------------------------------------------ 8. the device guards
@gpu
def test_a_clobbered_optim_state_or_a_family_state_of_another_shape_writes_nothing():
    ch = Chain("lstm")
    o = ch.optim_open({"max_norm": 1.0}, [1e-3], canaries=True)
    ch.fb(0)
    held = ch.buf[PAD:PAD + o["state"].numel()].clone()
    o["state"].fill_(CANARY)                              # as a buffer that uvad_optim_reset never filled
    before, whole = ch.state_bytes(), bytes(ch.buf.cpu().numpy())
    ch.optim(o)
    assert ch.state_bytes() == before and bytes(ch.buf.cpu().numpy()) == whole
    o["state"].copy_(held)                                # the optim state is good again; now the states carry another shape's P
    for h in (ch.hh, ch.hl):
        h["state"][16:20] = torch.tensor(list(np.asarray([h["P"] + 64], np.int32).tobytes()), dtype=torch.uint8, device=_dev())
    before, whole = ch.state_bytes(), bytes(ch.buf.cpu().numpy())
    ch.optim(o)
    assert ch.state_bytes() == before and bytes(ch.buf.cpu().numpy()) == whole and ch.canaries_intact()
    ch.rt.close()


# ------------------------------------------------------------------------------------------------ 9. the round trip
@gpu
def test_states_read_and_written_into_a_fresh_context_continue_to_the_uninterrupted_bytes():
    table = [1e-3, 2e-3, 3e-3, 2e-3, 1e-3, 5e-4]
    cfg = {"max_norm": 0.5, "weight_decay": 1e-2}
    whole = Chain("lstm", dropout=0.5)
    ow = whole.optim_open(cfg, table)
    first = Chain("lstm", dropout=0.5)
    of = first.optim_open(cfg, table)
    for k in range(3):
        whole.fb(k), whole.optim(ow)
        first.fb(k), first.optim(of)
    saved, rec = first.reads(), first.rt.optim_read(of)
    assert saved[1]["draws"] == 3 == first.rt.lstm_train_draws(first.hl) and saved[1]["scalars"].numel() == 10 and rec["step"] == 3
    second = Chain("lstm", dropout=0.5)                   # a fresh context: states reset from the initial weights, then written
    os_ = second.optim_open(cfg, table)
    second.rt.head_train_write(second.hh, saved[0])
    second.rt.lstm_train_write(second.hl, saved[1])
    second.rt.optim_write(os_, rec)
    assert second.state_bytes() == first.state_bytes() and bytes(os_["state"].cpu().numpy()) == bytes(of["state"].cpu().numpy())
    for k in range(3, 6):
        whole.fb(k), whole.optim(ow)
        second.fb(k), second.optim(os_)
    assert second.state_bytes() == whole.state_bytes() and second.rt.lstm_train_draws(second.hl) == 6
    assert bytes(os_["state"].cpu().numpy()) == bytes(ow["state"].cpu().numpy())
    for c in (whole, first, second):
        c.rt.close()


@gpu
def test_a_sincnet_state_round_trips_through_read_and_write():
    a = Chain("sincnet")
    o = a.optim_open({"max_norm": 1.0}, [1e-3])
    for k in range(2):
        a.fb(k), a.optim(o)
    b = Chain("sincnet")
    for h, r, write in zip(b.handles, a.reads(), (b.rt.head_train_write, b.rt.lstm_train_write, b.rt.sincnet_train_write)):
        write(h, r)
    sa, sb = a.snap(), b.snap()
    for x, y in zip(sa, sb):
        for key in ("w", "m", "v", "bc1", "bc2"):
            assert np.array_equal(_bits(x[key]), _bits(y[key])), key
        assert x["t"] == y["t"] == 2
    ob = b.optim_open({"max_norm": 1.0}, [1e-3])
    b.rt.optim_write(ob, a.rt.optim_read(o))
    a.fb(2), a.optim(o)
    b.fb(2), b.optim(ob)
    assert a.state_bytes() == b.state_bytes()             # the bank behind the Adam block too: the forward call rebuilt it from the masters
    a.rt.close(), b.rt.close()


# ------------------------------------------------------------------------------------------------ 10. train_vad
def _training_files(tmp_path):
    import wave
    from uvad_amd.synth import synth_pcm
    paths, labels = [], []
    for k in range(2):
        x = synth_pcm(1, 2 * 16000, seed=700 + k)[0]
        x[int(0.5 * 16000):int(1.0 * 16000)] *= 0.02
        p, f = tmp_path / f"t{k}.wav", tmp_path / f"t{k}.txt"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
        f.write_text("0.0\t0.5\tSPC\n1.0\t2.0\tSPC\n")
        paths.append(str(p)); labels.append(str(f))
    return paths, labels


def _train_config(tmp_path, files, where, epochs, **options):
    from config.config import load_config
    cfg = load_config()
    cfg.model_dict.encoding_dim = 64
    cfg.model_dict.lstm = {"hidden_size": 64, "num_layers": 2, "dropout": 0.5}
    cfg.model_dict.linear = {"hidden_size": 32, "num_layers": 1}
    cfg.input.kind, cfg.input.paths, cfg.input.labels = "wav", files[0], files[1]
    cfg.function, cfg.learning_rate, cfg.max_epochs, cfg.check_val_every_n_epoch = "train", 1e-2, epochs, 1
    cfg.window_seconds, cfg.max_duration, cfg.accumulate_grad_batches = 1.0, 2.0, 1
    cfg.experiments_dir = str(tmp_path / where)
    for k, v in options.items():
        cfg[k] = v
    return cfg


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    return a.dtype == b.dtype and a.shape == b.shape and bytes(a.contiguous().numpy()) == bytes(b.contiguous().numpy())


@gpu
def test_train_vad_with_every_option_resumes_to_the_bytes_of_the_uninterrupted_run(tmp_path):
    from uvad_amd.scripts import train_vad
    files = _training_files(tmp_path)
    options = dict(gradient_clip_val=1.0, weight_decay=1e-2, adamw=True, lr_schedule={"name": "cosine", "warmup_steps": 2})
    whole = train_vad(**_train_config(tmp_path, files, "whole", 4, **options))
    half = train_vad(**_train_config(tmp_path, files, "half", 4, stop_after_epoch=2, **options))
    assert half["checkpoint_path"].endswith("checkpoint-epoch=02.ckpt") and half["global_step"] * 2 == whole["global_step"]
    assert half["train_loss"] == whole["train_loss"][:2]
    rest = train_vad(**_train_config(tmp_path, files, "rest", 4, load_checkpoint=True, checkpoint_path=half["checkpoint_path"], **options))
    assert rest["train_loss"] == whole["train_loss"][2:] and rest["global_step"] == whole["global_step"]
    a, b = (torch.load(r["checkpoint_path"], weights_only=True) for r in (whole, rest))
    assert a["epoch"] == b["epoch"] == 4 and a["global_step"] == b["global_step"]
    assert _same(a["state_dict"], b["state_dict"]) and _same(a["optimizer_states"], b["optimizer_states"])
    assert set(a["optimizer_states"]) == {"head", "lstm", "optim"}
    rec = a["optimizer_states"]["optim"].numpy().view(np.uint32)
    assert int(rec[4]) == whole["global_step"] and int(rec[6]) == 0              # every step applied, none skipped


@gpu
def test_train_vad_without_the_options_runs_the_apply_path_as_before(tmp_path, monkeypatch):
    from uvad_amd.runtime import VadRuntime
    from uvad_amd.scripts import train_vad
    files = _training_files(tmp_path)
    calls = {"optim": 0, "apply": 0}
    step, apply = VadRuntime.optim_step, VadRuntime.lstm_train_apply
    monkeypatch.setattr(VadRuntime, "optim_step", lambda self, *a, **k: (calls.__setitem__("optim", calls["optim"] + 1), step(self, *a, **k))[1])
    monkeypatch.setattr(VadRuntime, "lstm_train_apply", lambda self, *a, **k: (calls.__setitem__("apply", calls["apply"] + 1), apply(self, *a, **k))[1])
    one = train_vad(**_train_config(tmp_path, files, "one", 2))
    assert calls == {"optim": 0, "apply": one["global_step"]}                     # the _apply calls, never the joint step
    two = train_vad(**_train_config(tmp_path, files, "two", 2))
    assert one["train_loss"] == two["train_loss"] and one["val_loss"] == two["val_loss"]
    a, b = (torch.load(r["checkpoint_path"], weights_only=True) for r in (one, two))
    assert _same(a["state_dict"], b["state_dict"]) and set(a) == {"state_dict", "epoch", "global_step", "optimizer_states"}
    # the joint step with everything off and a constant table is the _apply path, byte for byte
    calls["optim"] = calls["apply"] = 0
    off = train_vad(**_train_config(tmp_path, files, "off", 2, lr_schedule={"name": "constant"}))
    assert calls == {"optim": off["global_step"], "apply": 0}
    c = torch.load(off["checkpoint_path"], weights_only=True)
    assert off["train_loss"] == one["train_loss"] and _same(c["state_dict"], a["state_dict"])
    assert _same({k: c["optimizer_states"][k] for k in ("head", "lstm")}, a["optimizer_states"])


# ---------------------------------------------------------------- a state belongs to its family
# The smallest shapes the configure calls accept: a PyanNet of one unidirectional 64-unit LSTM layer and a 32 / 1 head behind the SincNet
# geometry of tests/test_gpu_sincnet_train.py; first_layer = the last layer, first_stage = 2; B = 2, S = 991 (one frame).
_FAMILIES = ("head", "lstm", "sincnet")
E_STATE = -3


@pytest.fixture(scope="module")
def family_handles():
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet(lstm={"hidden_size": 64, "num_layers": 1, "bidirectional": False, "dropout": 0.0}, linear={"hidden_size": 32, "num_layers": 1})
    m.build()
    seed_weights(m, 3, 1.0)
    sd = m.state_dict()
    with torch.no_grad():
        for k, v in SR.make_case(2, 991, 1)[0].items():
            sd["sincnet." + k].copy_(torch.from_numpy(np.ascontiguousarray(v, F32)))
    rt = m.runtime(_dev())
    hs = {"head": rt.head_train_open(segment=32), "lstm": rt.lstm_train_open(layers=1, segment=32),
          "sincnet": rt.sincnet_train_open(first_stage=2, segment=32)}
    # every state in a buffer as large as the largest, so that the size a foreign family is told is true
    big = max(h["state"].numel() for h in hs.values())
    for f, h in hs.items():
        h["state"] = torch.zeros(big, dtype=torch.uint8, device=_dev())
        rt._train_configure(h)
        rt._check(getattr(rt.lib, f"uvad_{f}_train_reset")(rt.ctx, h["state"].data_ptr(), big, None))
    return rt, hs, m


@gpu
@pytest.mark.parametrize("a,b", [(a, b) for a in _FAMILIES for b in _FAMILIES if a != b])
def test_a_state_of_one_family_is_refused_by_another(family_handles, a, b):
    rt, hs, _ = family_handles
    st, n = hs[a]["state"], hs[a]["state"].numel()
    torch.cuda.synchronize()
    before = st.clone()
    rt._train_configure(hs[b])                                                   # b is configured, and n is large enough for it
    assert n >= int(getattr(rt.lib, f"uvad_{b}_train_state_bytes")(rt.ctx))
    out = torch.zeros(max(h["out"].numel() for h in hs.values()), dtype=torch.float32, device=_dev())
    fn = lambda op: getattr(rt.lib, f"uvad_{b}_train_{op}")
    calls = {"apply": lambda: fn("apply")(rt.ctx, st.data_ptr(), n, None), "read": lambda: fn("read")(rt.ctx, st.data_ptr(), n, 0, out.data_ptr(), None),
             "write": lambda: fn("write")(rt.ctx, st.data_ptr(), n, 0, out.data_ptr(), None), "commit": lambda: fn("commit")(rt.ctx, st.data_ptr(), n)}
    for name, call in calls.items():
        assert call() == E_STATE, (name, rt.lib.uvad_last_error(rt.ctx))
        assert rt.lib.uvad_last_error(rt.ctx).decode() == f"uvad_{b}_train_{name}: call uvad_{b}_train_reset on this state first", name
    torch.cuda.synchronize()
    assert torch.equal(st, before) and not out.any()


@gpu
def test_the_shared_apply_reaches_each_family_with_its_own_state(family_handles):
    rt, hs, _ = family_handles
    wav = torch.from_numpy(SR.make_case(2, 991, 71)[1].astype(F32)).to(_dev())
    gt = torch.tensor([[1], [0]], dtype=torch.uint8, device=_dev())
    feats = rt.sincnet_train_forward(hs["sincnet"], wav)
    assert tuple(feats.shape) == (2, 1, 60)
    y = rt.lstm_train_forward(hs["lstm"], feats)
    _, gx = rt.head_train_grad(hs["head"], y, gt, want_grad_x=True)
    rt.sincnet_train_backward(hs["sincnet"], wav, rt.lstm_train_backward(hs["lstm"], feats, gx, want_grad_in=True))
    read = {"head": rt.head_train_read, "lstm": rt.lstm_train_read, "sincnet": rt.sincnet_train_read}
    apply = {"head": rt.head_train_apply, "lstm": rt.lstm_train_apply, "sincnet": rt.sincnet_train_apply}
    for f in _FAMILIES:
        r0 = read[f](hs[f])
        assert r0["step"] == 0 and r0["frames"] > 0 and np.abs(_flat(r0["grad"])).max() > 0, f
        apply[f](hs[f])
        r1 = read[f](hs[f])
        assert r1["step"] == 1 and r1["frames"] == 0 and not _flat(r1["grad"]).any(), f
        assert _flat(r1["weights"]).shape == _flat(r0["weights"]).shape == (hs[f]["P"],) and not np.array_equal(_flat(r1["weights"]), _flat(r0["weights"])), f
        for g in _FAMILIES:                                                       # ... and nobody else's
            if g != f:
                assert read[g](hs[g])["step"] == (1 if _FAMILIES.index(g) < _FAMILIES.index(f) else 0), (f, g)
