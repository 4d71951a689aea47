"""The reverberation stage on the device (uvad_reverb_*, include/uvad.h) against tests/reverb_ref.py: integer operands bit for bit at every
tile edge, general operands inside the forward-error bound of a K-term f32 sum, the plan word for word, pass-through of undrawn rows,
independence of the batch, the normalisation restated from the device's own z, the draw ordinal and graph replay, the refusals; then
the host layer (reverb_open / reverb_step, train_vad(reverb=...))."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import reverb_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG, E_STATE = -1, -3
SEED = 0x1234567887654321
GUARD = 256                                      # canary bytes on both sides of a guarded buffer
TILE, KC = 4096, 256                             # UVAD_REVERB_TILE, UVAD_REVERB_K_CHUNK (checked against the binding below)
# taps: the issue's list, and K + 31 (the offsets a chunk walks) one below / at / above one and two chunks of 256
KS = [1, 2, 31, 32, 33, 224, 225, 226, 255, 256, 257, 480, 481, 482, 513]
# lengths: the issue's list, and one below / at / above the output tile of a wave (1024) and of a workgroup (4096)
NS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 4099]
S = 4101                                         # > max n, odd: every second row starts 4 bytes off an 8-byte boundary


@pytest.fixture(scope="module")
def rt():
    from uvad_amd.runtime import VadRuntime
    from uvad_amd import _lib
    assert (_lib.REVERB_TILE, _lib.REVERB_K_CHUNK) == (TILE, KC)
    r = VadRuntime(DEV)                          # no feature tables, weights or model
    yield r
    r.close()


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


class Dev:
    """One reset state with guarded buffers, driven through the C ABI."""

    def __init__(self, rt, bank, first, prob=1.0, normalize=0, align=1, max_taps=0, seed=SEED, rows=len(NS), samples=S):
        from uvad_amd import _lib
        self.lib, self.ctx, self.L = rt.lib, rt.ctx, _lib
        self.rows, self.samples = rows, samples
        self.first = np.ascontiguousarray(first, np.int64)
        self.n_rirs = len(self.first) - 1
        self.bank = Guarded(4 * len(bank))
        self.bank.put(np.asarray(bank, np.float32))
        self.cfg = _lib.ReverbCfg(float(prob), int(normalize), int(align), int(max_taps), seed)
        self.state = Guarded(self.lib.uvad_reverb_state_bytes(C.byref(self.cfg), self.n_rirs))
        self.ws = Guarded(self.lib.uvad_reverb_ws_bytes(rows))
        self.plan = Guarded(16 * rows, fill=0x77)
        self.out = Guarded(4 * rows * samples, fill=0x77)
        assert self.state.n > 0 and self.ws.n > 0
        assert self.reset() == 0, self.err()

    def err(self):
        return self.lib.uvad_last_error(self.ctx).decode()

    def reset(self):
        return self.lib.uvad_reverb_reset(self.ctx, self.state.ptr, self.state.n, C.byref(self.cfg), self.bank.ptr,
                                          self.first.ctypes.data_as(C.POINTER(C.c_int64)), self.n_rirs, None)

    def call(self, d_in, fmt, nsamp, draw=None, row0=0, out=None, rows=None, samples=None, plan=True, stream=None):
        rows = self.rows if rows is None else rows
        head = (self.ctx, d_in, fmt, rows, self.samples if samples is None else samples, nsamp, self.out.ptr if out is None else out,
                self.plan.ptr if plan else None)
        tail = (self.state.ptr, self.state.n, self.ws.ptr, self.ws.n, stream)
        if draw is None:
            return self.lib.uvad_reverb_step(*head, *tail)
        return self.lib.uvad_reverb_apply(*head, row0, draw, *tail)

    def draws(self):
        return int(self.state.get(np.uint64)[7])

    def delays(self):
        pad = lambda v: (v + 255) // 256 * 256
        off = 256 + pad(8 * (self.n_rirs + 1)) + pad(4 * self.n_rirs)
        return self.state.get(np.uint8)[off:off + 4 * self.n_rirs].view(np.int32)

    def result(self, rows=None, samples=None):
        rows, samples = self.rows if rows is None else rows, self.samples if samples is None else samples
        torch.cuda.synchronize()
        return (self.out.get(np.float32)[:rows * samples].reshape(rows, samples), self.plan.get(np.int32)[:4 * rows].reshape(rows, 4))

    def intact(self):
        return all(g.intact() for g in (self.bank, self.state, self.ws, self.plan, self.out))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _nsamp(lens):
    return torch.tensor(list(lens), dtype=torch.int64, device=DEV)


def _int_rir(rng, K, peak_at):
    """Integer taps in [-7, 7] with the one largest, +-8, at peak_at."""
    h = rng.integers(-7, 8, K).astype(np.float32)
    h[peak_at] = 8.0 if peak_at % 2 else -8.0
    return h


def _decaying_rir(rng, K, peak_at):
    """Decaying noise with a unit direct path at peak_at."""
    h = (rng.standard_normal(K) * 0.3 * np.exp(-np.arange(K) / max(K / 4.0, 1.0))).astype(np.float32)
    h = np.clip(h, -0.9, 0.9)
    h[peak_at] = 1.0
    return h


@pytest.fixture(scope="module")
def rows_int():
    """len(NS) rows of integers in [-64, 64], row b valid over NS[b] samples; past it NaN (f32) / 32767 (int16)."""
    rng = np.random.default_rng(11)
    q = rng.integers(-64, 65, (len(NS), S)).astype(np.int16)
    x = q.astype(np.float32)
    for b, n in enumerate(NS):
        x[b, n:] = np.nan
        q[b, n:] = 32767
    return {"x": x, "q": q}


@pytest.fixture(scope="module")
def rows_f32():
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((len(NS), S)) * 0.1).astype(np.float32)
    for b, n in enumerate(NS):
        x[b, n:] = np.nan
    return x


@pytest.fixture(scope="module")
def srcs(rows_int, rows_f32):
    """The three batches on the device, uploaded once."""
    out = {}
    for name, a in (("xi", rows_int["x"]), ("qi", rows_int["q"]), ("xf", rows_f32)):
        out[name] = Guarded(a.nbytes)
        out[name].put(a)
    return out


# ---- 1. integer operands: every partial sum is an integer below 2^24 (x 2^-15 for int16), so every order is exact ---------------------------------
@pytest.mark.parametrize("K", KS)
def test_integer_operands_are_exact_at_every_tile_edge(rt, rows_int, srcs, K):
    """One response of K taps, its direct path at tap 0, mid and K - 1; rows of every length in NS (n < K and n <= d among them), f32 and
    int16, align 0 and 1: d_out equals the float64 restatement bit for bit."""
    rng = np.random.default_rng(100 + K)
    ns = _nsamp(NS)
    for peak in sorted({0, K // 2, K - 1}):
        h = _int_rir(rng, K, peak)
        for align in ((0, 1) if peak else (1,)):
            d = Dev(rt, h, [0, K], align=align)
            assert list(d.delays()) == [peak]
            for name, fmt in (("x", d.L.INGEST_F32), ("q", d.L.INGEST_I16)):
                assert d.call(srcs[name + "i"].ptr, fmt, ns.data_ptr(), draw=3) == 0, d.err()
                got, plan = d.result()
                want = rr.reverb(rows_int[name], NS, h, [0, K], 1.0, 0, align, 0, SEED, 3)
                assert plan.tobytes() == want["plan"].tobytes() and (plan[:, 0] == 1).all() and (plan[:, 2] == (peak if align else 0)).all()
                bad = np.argwhere(_bits(got) != _bits(want["out"]))
                assert not len(bad), (K, peak, align, name, bad[:5], got[tuple(bad[0])], want["out"][tuple(bad[0])])
            assert d.intact()
    assert all(g.intact() for g in srcs.values())


def _bank(rng, make, ks=KS):
    first = np.zeros(len(ks) + 1, np.int64)
    first[1:] = np.cumsum(ks)
    bank = np.concatenate([make(rng, K, [0, K // 2, K - 1][i % 3]) for i, K in enumerate(ks)])
    return bank, first


def test_integer_operands_from_a_bank_of_responses_and_a_cut_tail(rt, rows_int, srcs):
    """Rows draw their response from a bank (several rows share one); max_taps cuts the longer responses, and moves their delays."""
    bank, first = _bank(np.random.default_rng(21), _int_rir)
    ns = _nsamp(NS)
    for max_taps in (0, 100):
        d = Dev(rt, bank, first, max_taps=max_taps)
        assert np.array_equal(d.delays(), rr.delays(bank, first, max_taps))
        seen = []
        for draw in range(2):
            assert d.call(srcs["xi"].ptr, d.L.INGEST_F32, ns.data_ptr(), draw=draw) == 0, d.err()
            got, plan = d.result()
            want = rr.reverb(rows_int["x"], NS, bank, first, 1.0, 0, 1, max_taps, SEED, draw)
            assert plan.tobytes() == want["plan"].tobytes()
            assert np.array_equal(_bits(got), _bits(want["out"])), (max_taps, draw)
            seen += list(plan[:, 1])
        assert len(set(seen)) < len(seen) and len(set(seen)) > 4                 # shared responses, and several different ones
        assert d.intact()


# ---- 2. general operands: the forward-error bound of a K-term f32 sum in any order --------------------------------------------------------------
def test_general_operands_stay_inside_the_rigorous_bound(rt, rows_f32, srcs):
    """|z_i - z64_i| <= (K + 8) 2^-24 sum_k |h_k| |x_{i + d - k}|, the right side in float64: derived, not measured."""
    bank, first = _bank(np.random.default_rng(22), _decaying_rir)
    d = Dev(rt, bank, first)
    ns = _nsamp(NS)
    K = rr.taps(first)
    worst = 0.0
    for draw in range(3):
        assert d.call(srcs["xf"].ptr, d.L.INGEST_F32, ns.data_ptr(), draw=draw) == 0, d.err()
        got, plan = d.result()
        want = rr.reverb(rows_f32, NS, bank, first, 1.0, 0, 1, 0, SEED, draw)
        assert plan.tobytes() == want["plan"].tobytes()
        for b, n in enumerate(NS):
            lim = (int(K[plan[b, 1]]) + 8) * 2.0 ** -24 * want["absbound"][b]
            err = np.abs(got[b, :n].astype(np.float64) - want["z64"][b])
            if n:
                worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
            assert (err <= lim).all(), (draw, b, n, int(K[plan[b, 1]]), float((err - lim).max()))
            assert not _bits(got[b, n:]).any()
    print("largest error / bound:", worst)
    assert d.intact()


# ---- 3. the plan, pass-through, what lies past a length, guard bytes ---------------------------------------------------------------------------
def test_plan_and_pass_through(rt, rows_f32):
    bank, first = _bank(np.random.default_rng(23), _decaying_rir)
    x = rows_f32.copy()
    nan_payload = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    for b, n in enumerate(NS):
        if n > 2:
            x[b, 1], x[b, 2] = nan_payload, -0.0
    src = Guarded(x.nbytes)
    src.put(x)
    ns = _nsamp(NS)
    dly = rr.delays(bank, first)
    kinds = set()
    for prob in (0.0, 0.5, 1.0):
        for seed in (SEED, 7):
            d = Dev(rt, bank, first, prob=prob, seed=seed, normalize=1)
            for draw, row0 in ((0, 0), (5, 0), ((1 << 40) + 3, 9), (2, (1 << 32) - 4)):
                d.out.body()[:] = 0x77
                assert d.call(src.ptr, d.L.INGEST_F32, ns.data_ptr(), draw=draw, row0=row0) == 0, d.err()
                got, plan = d.result()
                want = rr.plan(len(NS), len(first) - 1, dly, prob, 1, seed, draw, row0)
                assert plan[:, :3].tobytes() == want[:, :3].tobytes(), (prob, seed, draw, row0)
                for b, n in enumerate(NS):
                    kinds.add(int(plan[b, 0]))
                    assert not _bits(got[b, n:]).any()                          # +0 past a length: the NaN there reached nothing
                    if not plan[b, 0]:
                        assert tuple(plan[b]) == (0, 0, 0, rr.ONE_BITS)
                        assert np.array_equal(_bits(got[b, :n]), _bits(x[b, :n]))   # the NaN's payload and -0 included
                if prob == 0.0:
                    assert not plan[:, 0].any()
                if prob == 1.0:
                    assert plan[:, 0].all()
            assert d.intact() and d.draws() == 0
    assert kinds == {0, 1} and src.intact()


def test_int16_rows_not_drawn_are_q_over_32768(rt, rows_int, srcs):
    d = Dev(rt, [1.0, 0.5], [0, 2], prob=0.0)
    assert d.call(srcs["qi"].ptr, d.L.INGEST_I16, _nsamp(NS).data_ptr()) == 0, d.err()
    got, plan = d.result()
    want = rr.reverb(rows_int["q"], NS, [1.0, 0.5], [0, 2], 0.0, 1, 1, 0, SEED, 0)
    assert np.array_equal(_bits(got), _bits(want["out"])) and plan.tobytes() == want["plan"].tobytes() and d.intact()


# ---- 4. rows are independent of the batch; the same call gives the same bits ---------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(rt, rows_f32, srcs):
    bank, first = _bank(np.random.default_rng(24), _decaying_rir)
    d = Dev(rt, bank, first, prob=0.7, normalize=1)
    ns = _nsamp(NS)
    assert d.call(srcs["xf"].ptr, d.L.INGEST_F32, ns.data_ptr(), draw=4) == 0, d.err()
    whole, plan = d.result()
    assert 0 < plan[:, 0].sum() < len(NS)
    assert d.call(srcs["xf"].ptr, d.L.INGEST_F32, ns.data_ptr(), draw=4) == 0, d.err()
    again, plan2 = d.result()
    assert np.array_equal(_bits(whole), _bits(again)) and plan.tobytes() == plan2.tobytes()           # the same call, the same bits
    for b in (0, 3, 9, 11, 12, 15):                                                                      # a one-row apply with row0 = b
        d.out.body()[:] = 0x77
        assert d.call(srcs["xf"].ptr + 4 * b * S, d.L.INGEST_F32, ns[b:].data_ptr(), draw=4, row0=b, rows=1) == 0, d.err()
        one, p1 = d.result(rows=1)
        assert np.array_equal(_bits(one[0]), _bits(whole[b])) and p1[0].tobytes() == plan[b].tobytes(), b
    lo, hi, S2 = 9, 14, S + 7                                                                            # another B and another S
    wide = np.full((hi - lo, S2), np.nan, np.float32)
    wide[:, :S] = rows_f32[lo:hi]
    src = Guarded(wide.nbytes)
    src.put(wide)
    d2 = Dev(rt, bank, first, prob=0.7, normalize=1, rows=hi - lo, samples=S2)
    assert d2.call(src.ptr, d2.L.INGEST_F32, ns[lo:].data_ptr(), draw=4, row0=lo) == 0, d2.err()
    part, pp = d2.result()
    assert pp.tobytes() == plan[lo:hi].tobytes() and np.array_equal(_bits(part[:, :S]), _bits(whole[lo:hi])) and not _bits(part[:, S:]).any()
    assert d.intact() and d2.intact() and src.intact()


# ---- 5. normalisation, restated from the device's own z -------------------------------------------------------------------------------------------
def test_normalisation_is_one_rounding_of_z_times_g(rt, rows_f32):
    bank, first = _bank(np.random.default_rng(25), _decaying_rir)
    x = rows_f32.copy()
    x[5, :NS[5]] = 0.0                                                           # an all-zero row: g = 1 and zeros
    src = Guarded(x.nbytes)
    src.put(x)
    ns = _nsamp(NS)
    raw, nrm = Dev(rt, bank, first, normalize=0), Dev(rt, bank, first, normalize=1)
    assert raw.call(src.ptr, raw.L.INGEST_F32, ns.data_ptr(), draw=1) == 0, raw.err()
    z, pz = raw.result()
    assert nrm.call(src.ptr, nrm.L.INGEST_F32, ns.data_ptr(), draw=1) == 0, nrm.err()
    got, plan = nrm.result()
    want = rr.reverb(x, NS, bank, first, 1.0, 1, 1, 0, SEED, 1, z_dev=z)
    assert (pz[:, 3] == rr.ONE_BITS).all() and plan.tobytes() == want["plan"].tobytes()
    assert np.array_equal(_bits(got), _bits(want["out"]))
    gains = plan[:, 3].copy().view(np.float32)
    print("gains", gains)
    assert gains[5] == 1.0 and not _bits(got[5]).any() and gains[0] == 1.0 and len(set(gains.tolist())) > 8
    assert raw.intact() and nrm.intact() and src.intact()


# ---- 6. the ordinal, a captured graph, the delays -------------------------------------------------------------------------------------------------
def test_step_advances_the_ordinal_and_a_graph_draws_anew(rt, rows_f32, srcs):
    bank, first = _bank(np.random.default_rng(26), _decaying_rir)
    ns = _nsamp(NS)
    off = Dev(rt, bank, first, prob=0.0)
    for i in range(2):
        assert off.call(srcs["xf"].ptr, off.L.INGEST_F32, ns.data_ptr()) == 0, off.err()
    torch.cuda.synchronize()
    assert off.draws() == 2                                                      # also at prob 0
    d = Dev(rt, bank, first, prob=0.5, normalize=1)
    want = []
    for draw in range(3):
        assert d.call(srcs["xf"].ptr, d.L.INGEST_F32, ns.data_ptr(), draw=draw) == 0, d.err()
        want.append(d.result())
    assert d.draws() == 0 and len({p.tobytes() for _, p in want}) == 3
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert d.call(srcs["xf"].ptr, d.L.INGEST_F32, ns.data_ptr(), stream=C.c_void_p(s.cuda_stream)) == 0, d.err()
    torch.cuda.synchronize()
    assert d.draws() == 0                                                        # capture enqueues nothing
    for i in range(3):
        g.replay()
        got, plan = d.result()
        assert plan.tobytes() == want[i][1].tobytes() and np.array_equal(_bits(got), _bits(want[i][0])) and d.draws() == i + 1, i
    assert d.reset() == 0 and d.draws() == 0 and d.intact()


def test_delays_with_ties_and_a_nan_tap(rt):
    rirs = [[0.5, -1.0, 1.0, 0.25], [np.nan, 0.5, np.nan, 0.5], [0.0, 0.0, 0.0], [np.nan, np.nan], [-3.0],
            list(np.r_[np.zeros(700), 2.0, np.zeros(300), -2.0, np.zeros(40)]), list(np.r_[np.ones(513)])]
    first = np.r_[0, np.cumsum([len(h) for h in rirs])]
    bank = np.concatenate([np.asarray(h, np.float32) for h in rirs])
    d = Dev(rt, bank, first, rows=1)
    assert list(d.delays()) == list(rr.delays(bank, first)) == [1, 1, 0, 0, 0, 700, 0]
    cut = Dev(rt, bank, first, max_taps=2, rows=1)
    assert list(cut.delays()) == list(rr.delays(bank, first, 2)) == [1, 1, 0, 0, 0, 0, 0]
    assert d.intact() and cut.intact()


# ---- 7. refusals that need a context: nothing is enqueued -----------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(rt, srcs):
    bank, first = _bank(np.random.default_rng(27), _decaying_rir)
    d = Dev(rt, bank, first)
    lib, ctx, L = d.lib, d.ctx, d.L
    ns = _nsamp(NS)
    firstp = lambda a: np.ascontiguousarray(a, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    cfg = lambda **kw: L.ReverbCfg(*[kw.get(k, v) for k, v in (("prob", 0.5), ("normalize", 1), ("align", 1), ("max_taps", 0), ("seed", 1))])

    def reset(cfg_=None, state=None, nbytes=None, bank_=None, first_=d.first, n_rirs=None, cfgp=True):
        return lib.uvad_reverb_reset(ctx, d.state.ptr if state is None else state, d.state.n if nbytes is None else nbytes,
                                     C.byref(d.cfg if cfg_ is None else cfg_) if cfgp else None, d.bank.ptr if bank_ is None else bank_,
                                     None if first_ is None else firstp(first_), d.n_rirs if n_rirs is None else n_rirs, None)

    n1 = len(first)
    huge = [0] + [(1 << 20) + 1 + i for i in range(n1 - 1)]
    for kw in (dict(state=0), dict(bank_=0), dict(first_=None), dict(cfgp=False), dict(state=d.state.ptr + 8), dict(bank_=d.bank.ptr + 2),
               dict(cfg_=cfg(prob=-0.1)), dict(cfg_=cfg(prob=1.5)), dict(cfg_=cfg(prob=math.nan)), dict(cfg_=cfg(prob=math.inf)),
               dict(cfg_=cfg(max_taps=-1)), dict(n_rirs=0), dict(first_=[0, 1, 1] + list(range(2, n1 - 1))),
               dict(first_=[0, 5, 4] + list(range(6, n1 + 3))), dict(first_=list(range(1, n1 + 1))), dict(first_=huge), dict(nbytes=d.state.n - 1)):
        assert reset(**kw) == E_ARG, kw
    assert lib.uvad_reverb_reset(None, d.state.ptr, d.state.n, C.byref(d.cfg), d.bank.ptr, firstp(d.first), d.n_rirs, None) == E_ARG

    def step(apply, d_in=srcs["xf"].ptr, fmt=L.INGEST_F32, rows=len(NS), samples=S, out=d.out.ptr, state=d.state.ptr, sbytes=d.state.n, ws=d.ws.ptr,
             wbytes=d.ws.n, plan=d.plan.ptr, ctx=ctx):
        head = (ctx, d_in, fmt, rows, samples, ns.data_ptr(), out, plan)
        tail = (state, sbytes, ws, wbytes, None)
        return lib.uvad_reverb_apply(*head, 0, 0, *tail) if apply else lib.uvad_reverb_step(*head, *tail)

    # a context knows the states IT reset, by address: this one has reset none (a fresh buffer may reuse the address of an earlier test's state)
    from uvad_amd.runtime import VadRuntime
    other = VadRuntime(DEV)
    for apply in (False, True):
        for kw in (dict(d_in=0), dict(out=0), dict(state=0), dict(ws=0), dict(state=d.state.ptr + 8), dict(ws=d.ws.ptr + 4), dict(fmt=2), dict(fmt=-1),
                   dict(rows=0), dict(samples=0), dict(samples=1 << 31), dict(sbytes=d.state.n - 1), dict(wbytes=d.ws.n - 1), dict(out=d.out.ptr + 2),
                   dict(d_in=srcs["xf"].ptr + 2), dict(plan=d.plan.ptr + 2), dict(d_in=d.out.ptr), dict(fmt=L.INGEST_I16, d_in=d.out.ptr)):
            assert step(apply, **kw) == E_ARG, (apply, kw)
        assert step(apply, ctx=other.ctx) == E_STATE and "uvad_reverb_reset" in lib.uvad_last_error(other.ctx).decode()
    other.close()
    torch.cuda.synchronize()
    assert d.intact() and d.draws() == 0
    assert (d.out.get(np.uint8) == 0x77).all() and (d.plan.get(np.uint8) == 0x77).all()


# ---- 8. the host layer ---------------------------------------------------------------------------------------------------------------------------
def test_reverb_open_and_reverb_step(rt, rows_int):
    from uvad_amd.synth import rir
    ks = [33, 257, 513]
    bank, first = _bank(np.random.default_rng(28), _int_rir, ks)
    st = rt.reverb_open(bank, ks, prob=1.0, normalize=False, align=True, seed=SEED)
    assert list(rt.reverb_delays(st)) == list(rr.delays(bank, first))
    x = torch.from_numpy(rows_int["x"]).to(DEV)
    out, plan = rt.reverb_step(st, x, nsamp=NS, plan=True)
    want = rr.reverb(rows_int["x"], NS, bank, first, 1.0, 0, 1, 0, SEED, 0)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want["out"])) and plan.cpu().numpy().tobytes() == want["plan"].tobytes()
    q = torch.from_numpy(rows_int["q"]).to(DEV)
    out = rt.reverb_step(st, q, nsamp=torch.tensor(NS, device=DEV))
    want = rr.reverb(rows_int["q"], NS, bank, first, 1.0, 0, 1, 0, SEED, 1)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want["out"])) and rt.reverb_draws(st) == 2
    y = torch.empty_like(x)
    assert rt.reverb_step(st, x, nsamp=NS, out=y, draw=0, row0=0) is y and rt.reverb_draws(st) == 2
    with pytest.raises(RuntimeError):
        rt.reverb_step(st, x, out=x)                                             # d_out == d_in is refused
    for bad in (dict(rir_lengths=[3, 0, 5]), dict(rir_lengths=ks, prob=1.5), dict(rir_lengths=ks, max_taps=-1)):
        with pytest.raises(ValueError):
            rt.reverb_open(bank, **bad)
    with pytest.raises(ValueError):
        rt.reverb_open(bank[:10], ks)
    h = rir(800, 0.02, 40, seed=3)
    assert h.dtype == np.float32 and h.shape == (800,) and h[40] == 1.0 and rr.delay(h) == 40 and not h[:40].any()
    assert np.array_equal(h, rir(800, 0.02, 40, seed=3)) and not np.array_equal(h, rir(800, 0.02, 40, seed=4))
    assert np.abs(h[600:]).max() < 0.1 * np.abs(h[41:200]).max()                 # it decays


def _wav(path, x):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
    return str(path)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """Two speech-like recordings with label files, two noise files and two impulse responses."""
    from uvad_amd.synth import rir, synth_pcm
    d = tmp_path_factory.mktemp("reverb_corpus")
    paths, labels = [], []
    for k in range(2):
        x = synth_pcm(1, int(1.2 * 16000) + 300 * (1 - k), seed=700 + k)[0]
        x[int(0.3 * 16000):int(0.6 * 16000)] *= 0.02
        paths.append(_wav(d / f"a{k}.wav", x))
        (d / f"a{k}.txt").write_text("0.0\t0.3\tSPC\n0.6\t1.2\tSPC\n")
        labels.append(str(d / f"a{k}.txt"))
    rng = np.random.default_rng(5)
    noise = [_wav(d / "n0.wav", rng.standard_normal(5000) * 0.2), _wav(d / "n1.wav", rng.standard_normal(30000) * 0.05)]
    rirs = [_wav(d / "r0.wav", 0.9 * rir(1500, 0.15, 20, seed=1)), _wav(d / "r1.wav", 0.9 * rir(3000, 0.3, 50, seed=2))]
    return {"dir": d, "paths": paths, "labels": labels, "noise": noise, "rirs": rirs}


def _train_cfg(corpus, front, where, noise=None, reverb=None):
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
    cfg.function, cfg.learning_rate, cfg.max_epochs, cfg.check_val_every_n_epoch = "train", 1e-2, 1, 1
    cfg.window_seconds, cfg.max_duration, cfg.accumulate_grad_batches = 0.4, 0.8, 1
    cfg.experiments_dir = str(corpus["dir"] / where)
    cfg.noise, cfg.reverb = noise, reverb
    return cfg


def _ckpt_bytes(run):
    """Every tensor of the checkpoint's state_dict, as bytes."""
    sd = torch.load(run["checkpoint_path"], map_location="cpu", weights_only=True)["state_dict"]
    return b"".join(k.encode() + sd[k].contiguous().numpy().tobytes() for k in sorted(sd))


@pytest.mark.parametrize("front", ["fbank", "sincnet"])
def test_train_vad_with_reverb(corpus, front):
    from uvad_amd.scripts import train_vad
    reverb = {"paths": corpus["rirs"], "prob": 1.0, "max_seconds": 0.15}
    noise = {"paths": corpus["noise"], "snr": (10, 20), "mix_prob": 0.5}
    clean = train_vad(**_train_cfg(corpus, front, front + "_clean"))
    got = train_vad(**_train_cfg(corpus, front, front + "_reverb", reverb=reverb))
    for run in (clean, got):
        assert len(run["train_loss"]) == 1 and np.isfinite(run["train_loss"]).all() and np.isfinite([l for _, l in run["val_loss"]]).all()
    assert got["train_loss"] != clean["train_loss"] and _ckpt_bytes(got) != _ckpt_bytes(clean)
    none = train_vad(**_train_cfg(corpus, front, front + "_none", reverb=None))
    assert none["train_loss"] == clean["train_loss"] and _ckpt_bytes(none) == _ckpt_bytes(clean)      # reverb = None: today's run
    noisy = train_vad(**_train_cfg(corpus, front, front + "_noise", noise=noise))
    both_off = train_vad(**_train_cfg(corpus, front, front + "_noise_r0", noise=dict(noise), reverb={"prob": 0}))
    assert both_off["train_loss"] == noisy["train_loss"] and _ckpt_bytes(both_off) == _ckpt_bytes(noisy)   # prob 0: the stage changes no bit
    both = train_vad(**_train_cfg(corpus, front, front + "_both", noise=dict(noise), reverb=dict(reverb)))
    assert both["train_loss"] != noisy["train_loss"] and np.isfinite(both["train_loss"]).all()
    with pytest.raises(ValueError, match="paths"):
        train_vad(**_train_cfg(corpus, front, front + "_bad", reverb={"prob": 0.5}))
