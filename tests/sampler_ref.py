"""The sampler stage (uvad_sampler_*, include/uvad.h) restated in numpy: the epoch permutation, the window table, the plan of a step, the
gather and the labels.  Everything is integer or a copy, so the device's bytes equal these."""
import numpy as np

from lstm_dropout_ref import philox4x32_10

FBANK, SINCNET = 0, 1
PLAN_WORDS = 8
TAG_PERM, TAG_SET = 0x53500000, 0x53440000


def perm_params(N):
    k = max(8, int(N - 1).bit_length())
    k += k & 1
    return k, k // 2, (1 << (k // 2)) - 1


def perm_all(N, seed, d, e, shuffle=True):
    """perm(N, seed, d, e, p) for every p < N, as an int64 array (the walk vectorised: every element is walked until it is below N).
    e: one epoch -> (N,), or an array of E epochs -> (E, N)."""
    es = np.array([e] if np.isscalar(e) else e, dtype=np.uint64)
    x = np.tile(np.arange(N, dtype=np.uint64), len(es))
    ee = np.repeat(es, N)
    if shuffle and N > 1:
        _, half, mask = perm_params(N)
        half, mask = np.uint64(half), np.uint64(mask)
        key = (seed & 0xFFFFFFFF, seed >> 32)
        todo = np.arange(x.size)
        while todo.size:
            v, ev = x[todo], ee[todo]
            L, R = v >> half, v & mask
            for t in range(4):
                F = philox4x32_10((R | np.uint64(t << 16), np.uint64(TAG_PERM | d), ev & np.uint64(0xFFFFFFFF), ev >> np.uint64(32)), key)[0]
                L, R = R, L ^ (F.astype(np.uint64) & mask)
            x[todo] = (L << half) | R
            todo = todo[x[todo] >= np.uint64(N)]
    x = x.astype(np.int64)
    return x if np.isscalar(e) else x.reshape(len(es), N)


def perm(N, seed, d, e, p, shuffle=True):
    """One value, by the scalar walk (what a device thread does)."""
    if not shuffle or N <= 1:
        return int(p)
    _, half, mask = perm_params(N)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    x = int(p)
    while True:
        L, R = x >> half, x & mask
        for t in range(4):
            F = int(philox4x32_10((R | t << 16, TAG_PERM | d, e & 0xFFFFFFFF, e >> 32), key)[0])
            L, R = R, L ^ (F & mask)
        x = L << half | R
        if x < N:
            return x


def window_table(rec_lengths, W, min_keep, rec_set=None, D=1):
    """-> (windows (N, 3) int64 {recording, start, n} in table order, first [D + 1]): grouped by dataset, recording order inside one."""
    rec_set = [0] * len(rec_lengths) if rec_set is None else list(rec_set)
    rows, first = [], [0]
    for d in range(D):
        for r, n_r in enumerate(rec_lengths):
            if rec_set[r] != d:
                continue
            k = 0
            while k * W < n_r:
                n = min(W, n_r - k * W)
                if n > min_keep:
                    rows.append((r, k * W, n))
                k += 1
        first.append(len(rows))
    return np.array(rows, np.int64).reshape(-1, 3), np.array(first, np.int64)


def cum_table(weights):
    w = np.asarray(weights, np.float64)
    part = np.cumsum(w)                                # left to right
    cum = [int(np.floor(part[d] / part[-1] * 4294967296.0)) for d in range(len(w))]
    cum[-1] = 1 << 32
    return cum


def frames_fbank(n, frame_len=400, hop=160, snip_edges=False):
    return (0 if n < frame_len else 1 + (n - frame_len) // hop) if snip_edges else (n + hop // 2) // hop


def frames_sincnet(n, kw=(251, 5, 5), stride=10):
    L = n
    for i in range(3):
        lconv = (L - kw[i]) // (stride if i == 0 else 1) + 1 if L >= kw[i] else 0
        L = lconv // 3
    return L


class Sampler:
    """The state of uvad_sampler_reset and its step / apply.  frames: n samples -> frames (the front end's count)."""

    def __init__(self, pcm, rec_lengths, sups, W, min_keep, geometry, frames, hop=160, half=496, step=270, rec_set=None, weights=(1.0,),
                 shuffle=True, drop_last=False, pad=False, batch=0, seed=0):
        self.pcm = np.asarray(pcm)
        self.first = np.concatenate([[0], np.cumsum(rec_lengths)]).astype(np.int64)
        self.sups = [np.asarray(s, np.int64).reshape(-1, 2) for s in sups]       # per recording
        self.W, self.geometry, self.frames, self.hop, self.sinc_half, self.sinc_step = W, geometry, frames, hop, half, step
        self.D = len(weights)
        self.windows, self.set_first = window_table(rec_lengths, W, min_keep, rec_set, self.D)
        self.N = np.diff(self.set_first)
        assert (self.N > 0).all()
        self.L = self.N.copy()
        if drop_last:
            assert self.D == 1 and self.N[0] >= batch
            self.L[0] = self.N[0] // batch * batch
        self.cum = cum_table(weights)
        self.shuffle, self.pad, self.seed = shuffle, pad, seed
        self.cursor, self.draws = np.zeros(self.D, np.int64), 0
        self.T = frames(W)
        self._perms = {}

    def _perm(self, d, e, p):
        key = (d, e)
        if key not in self._perms:
            self._perms[key] = perm_all(int(self.N[d]), self.seed, d, e, self.shuffle)
        return int(self._perms[key][p])

    def datasets(self, B, draw, row0=0):
        w0 = philox4x32_10((np.arange(row0, row0 + B, dtype=np.uint64), TAG_SET, draw & 0xFFFFFFFF, draw >> 32),
                           (self.seed & 0xFFFFFFFF, self.seed >> 32))[0].astype(np.uint64)
        return np.array([next(d for d in range(self.D) if int(v) < self.cum[d]) for v in w0], np.int64)

    def apply(self, B, cursor, draw, row0=0):
        """-> dict(plan (B, 8) int32, out (B, W) f32, nsamp (B,) int64, labels (B, T) uint8, frames (B,) int32, counts (D,))"""
        ds = self.datasets(B, draw, row0)
        plan = np.zeros((B, PLAN_WORDS), np.int32)
        out = np.zeros((B, self.W), np.float32)
        nsamp, frames = np.zeros(B, np.int64), np.zeros(B, np.int32)
        labels = np.zeros((B, self.T), np.uint8)
        counts = np.zeros(self.D, np.int64)
        for b in range(B):
            d = int(ds[b])
            c = int(cursor[d]) + int(counts[d])
            counts[d] += 1
            e, p = divmod(c, int(self.L[d]))
            w = int(self.set_first[d]) + self._perm(d, e, p)
            r, start, n = (int(v) for v in self.windows[w])
            length = self.W if self.pad else n
            Tb = self.frames(length)
            plan[b] = d, np.uint32(e & 0xFFFFFFFF).astype(np.int32), p, w, r, start, n, Tb
            src = self.pcm[self.first[r] + start:self.first[r] + start + n]
            if src.dtype == np.int16:
                out[b, :n] = src.astype(np.float32) * np.float32(1.0 / 32768.0)
            else:
                out[b, :n].view(np.uint32)[:] = src.view(np.uint32)                 # bit for bit
            nsamp[b], frames[b] = length, Tb
            for s, t in self.sups[r]:
                rs, re = max(int(s) - start, 0), min(int(t) - start, n)
                if re <= rs:
                    continue
                if self.geometry == FBANK:
                    st, et = rs // self.hop, re // self.hop
                else:
                    st = max((rs - self.sinc_half) // self.sinc_step, 0) if rs > 0 else 0
                    et = max((re - self.sinc_half) // self.sinc_step, 0) if re < length else Tb
                labels[b, st:min(et, Tb)] = 1
        return dict(plan=plan, out=out, nsamp=nsamp, labels=labels, frames=frames, counts=counts)

    def step(self, B):
        res = self.apply(B, self.cursor, self.draws)
        self.cursor = self.cursor + res["counts"]
        self.draws += 1
        return res
