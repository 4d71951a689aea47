"""A plain-loop restatement of the group gate's step rule (uvad_gate_group_*, include/uvad.h) and its offline definition, written from the
header and sharing nothing with uvad_amd: one label at a time, samples and best bytes by their positions.  The offline definition stands on
tests/cuts_ref.py's table and tests/fuse_ref.py's pick.  tests/test_gate_group_ref.py proves the step against the definition on whole
sessions; the GPU tests compare every step's bytes with the step."""
import numpy as np

import cuts_ref
import fuse_ref
from gate_ref import END, FIRST, IDLE, INT_MAX, LAST, LOST, OPEN, PENDING, SEG_DTYPE, SHORT, START, assemble, max_out as gate_max_out, max_seg  # noqa: F401

UNSYNC = 16                                    # UVAD_GATE_UNSYNC
MAX_DECIDE = 1 << 24


def channel(flags):
    """UVAD_GATE_CHANNEL."""
    return (int(flags) >> 8) & 0xff


def history(cfg, lag, chunk, D):
    """uvad_gate_group_history: chunk + (lag + pad + D) hop + lead."""
    pad, max_len, min_len, hop, lead, tail = cfg
    return chunk + (lag + pad + D) * hop + lead


def best_history(cfg, lag, chunk, D):
    """uvad_gate_group_best_history: ceil(chunk / hop) + lag + pad + D."""
    pad, max_len, min_len, hop, lead, tail = cfg
    return -(-chunk // hop) + lag + pad + D


def max_out(cfg, ld_lab, chunk, D):
    """uvad_gate_group_max_out: uvad_gate_max_out + D hop."""
    return gate_max_out(cfg, ld_lab, chunk) + D * cfg[3]


def state_bytes(G, N, unit, hist, best_hist):
    r16 = lambda v: (v + 15) // 16 * 16
    return 256 + G * (96 + r16(best_hist)) + N * r16(hist * unit)


class Group:
    """One group of M members, step by step.  cfg = (pad, max_len, 0, hop, lead, tail); hist: samples each member's ring holds; best_hist:
    bytes the best ring holds; D: the decision horizon."""

    def __init__(self, cfg, M, hist, best_hist, D, dtype=np.int16):
        self.pad, self.W, min_len, self.hop, self.lead, self.tail = (int(v) for v in cfg)
        assert min_len == 0 and M >= 1 and D >= 1
        self.M, self.H, self.BH, self.D, self.dtype = int(M), int(hist), int(best_hist), int(D), np.dtype(dtype)
        self.rings = np.zeros((self.M, self.H), self.dtype)
        self.bring = np.zeros(self.BH, np.uint8)
        self.wp = self.bwp = 0      # the rings' write positions: they run on across sessions
        self.live = False
        self._clear()
        self.trace = set()
        self.deep_pcm = self.deep_best = 0      # the deepest reads so far: places behind the newest sample / best byte
        self.voteless = 0                       # frames of a choice window that could not vote

    def _clear(self):
        self.A = self.F = self.Fb = 0
        self.mode, self.c = IDLE, 0
        self.pf = self.idx = self.sent = 0
        self.started, self.ch, self.unsync = False, 0, False

    def _pick(self, f, w):
        counts = [0] * self.M
        for t in range(f, f + w):
            back = self.Fb - t
            if back < 1 or back > self.BH:
                self.voteless += 1
                continue
            self.deep_best = max(self.deep_best, back)
            b = int(self.bring[(self.bwp - back) % self.BH])
            if b < self.M:
                counts[b] += 1
        return max(range(self.M), key=lambda i: (counts[i], -i))

    def _record(self, flags, k, upto):
        if not self.started and not flags & LAST and k < self.D:
            self.trace.add("deferred")
            return                                                          # the first D frames are not all known yet
        first = max(self.pf * self.hop - self.lead, 0)
        total = max(upto - first, 0)
        n = max(total - self.sent, 0)
        if not flags & LAST and n == 0:
            return
        src = first + self.sent
        if not self.started:
            flags |= FIRST
            self.ch = self._pick(self.pf, min(k, self.D))                   # the one place a channel is chosen
            if self.pf < self.F_before:
                self.trace.add("backlog")
        flags |= self.ch << 8
        if self.unsync:
            flags |= UNSYNC
        if n > 0:
            self.deep_pcm = max(self.deep_pcm, self.A - src)
            if src < self.A - self.H:
                flags |= LOST
        self.recs.append((self.idx, flags, self.pf, k, self.sent, n, src, self.ch))
        self.sent, self.started = total, True

    def _close(self, k, ending):
        want = (self.pf + k) * self.hop + self.tail
        if k < self.D:
            self.trace.add("closed below D")
        self._record(LAST | (SHORT if (not ending and self.A < want) else 0), k, min(want, self.A))
        self.idx += 1
        self.pf += k
        self.sent, self.started = 0, False

    def _cover(self, g, ending):
        while self.W and g - self.pf >= self.W:
            self.trace.add("split")
            self._close(self.W, ending)

    def _known(self):
        return self.F if self.mode == OPEN else min(self.c + self.pad, self.F)

    def step(self, chunks, best, labels, flags, ld_out, max_seg_, differ=False):
        """chunks (M, chunk): the members' samples of this step; best: the step's best bytes; labels: the labels finalised by this step;
        flags: the group's START / END bits; differ: the members' flag bytes differ in this step -> (out (ld_out,), seg records, count)."""
        out = np.zeros(ld_out, self.dtype)
        self.recs = []
        if flags & START:
            self._clear()
            self.live = True
        if not self.live:
            return out, np.zeros(0, SEG_DTYPE), 0
        self.unsync = self.unsync or bool(differ)
        ending = bool(flags & END)
        chunks = np.asarray(chunks, self.dtype).reshape(self.M, -1)
        n = chunks.shape[1]
        self.rings[:, (self.wp + np.arange(n)) % self.H] = chunks           # commit, then read
        self.wp = (self.wp + n) % self.H
        self.A += n
        for v in np.asarray(best, np.uint8).tolist():
            self.bring[self.bwp] = v
            self.bwp = (self.bwp + 1) % self.BH
            self.Fb += 1
        self.F_before = self.F
        for v in np.asarray(labels).tolist():
            if self.F >= INT_MAX:
                break
            t, v = self.F, bool(v)
            if self.mode == IDLE and v:
                self.pf, self.mode = max(t - self.pad, 0), OPEN
            elif self.mode == OPEN and not v:
                self.c, self.mode = t, PENDING
            elif self.mode == PENDING and v:
                self.mode = OPEN
            self.F = t + 1
            if self.mode == PENDING and not v and t >= self.c + 2 * self.pad:
                hi = self.c + self.pad
                self._cover(hi, ending)
                if hi > self.pf:
                    self._close(hi - self.pf, ending)
                self.mode = IDLE
            elif self.mode != IDLE:
                self._cover(self._known(), ending)
        if self.mode != IDLE:
            g = self._known()
            if ending:
                self._cover(g, True)
                if g > self.pf:
                    self._close(g - self.pf, True)
            elif g > self.pf:
                self._record(0, g - self.pf, min(g * self.hop, self.A))
        seg, off = [], 0
        for r, (idx, fl, f, k, offset, n, src, ch) in enumerate(self.recs):
            if r >= max_seg_:
                break
            ns = min(n, ld_out - off)
            p = src + np.arange(ns)
            at = (self.wp - (self.A - p)) % self.H
            out[off:off + ns] = np.where(p >= self.A - self.H, self.rings[ch][at], 0)
            seg.append((idx, fl, f, k, offset, n, ns))
            off += ns
        count = len(self.recs)
        if ending:
            self._clear()
            self.live = False
        return out, np.array(seg, SEG_DTYPE).reshape(-1), count


def offline(labels, best, audio, cfg, D):
    """The definition on a whole session: labels (n,) the group's fused labels, best (n,) its best bytes, audio (M, S) the members' samples.
    -> [(first_frame, n_frames, position, samples)]: cuts_ref's table on the labels, fuse_ref's pick on each cut truncated to its first
    D frames, each cut gathered from the picked member's row."""
    audio = np.asarray(audio)
    M, S = audio.shape
    tab, _ = cuts_ref.table(np.asarray(labels, np.uint8)[None, :], None, None, S, cfg)
    trunc = [(0, int(c["index"]), int(c["first_frame"]), min(int(c["n_frames"]), D), 0, 0) for c in tab]
    _, picks = fuse_ref.pick_ref(np.asarray(best, np.uint8)[None, :], [list(range(M))], trunc)
    return [(int(c["first_frame"]), int(c["n_frames"]), p, audio[p, int(c["first_sample"]):int(c["first_sample"]) + int(c["n_samples"])])
            for c, p in zip(tab, picks)]


def run_session(group, audio, best, labels, chunk, frontier, ld_out, max_seg_, differ=()):
    """One session through `group`: step s takes samples [s chunk, (s + 1) chunk) of audio (M, S), S a multiple of chunk, and the labels
    and best bytes up to frontier[s] = (F, Fb) (the last step: all of them), with START on the first step and END on the last.
    -> per step (out, seg, count)."""
    M, S = audio.shape
    steps = S // chunk
    assert steps * chunk == S and len(frontier) == steps and tuple(frontier[-1]) == (len(labels), len(best))
    res, F0, B0 = [], 0, 0
    for s in range(steps):
        F1, B1 = frontier[s]
        fl = (START if s == 0 else 0) | (END if s == steps - 1 else 0)
        res.append(group.step(audio[:, s * chunk:(s + 1) * chunk], best[B0:B1], labels[F0:F1], fl, ld_out, max_seg_, s in differ))
        F0, B0 = F1, B1
    return res


def session_cuts(res):
    """run_session's result -> [(first_frame, n_frames, flags or-ed, samples, done)] through gate_ref.assemble, after checking that every
    record of a cut names one channel."""
    recs = []
    for out, seg, count in res:
        assert count == len(seg), "a record was dropped: max_seg too small for this check"
        off = 0
        for r in seg:
            recs.append((r, out[off:off + int(r["n_stored"])]))
            off += int(r["n_stored"])
    chans = {}
    for r, _ in recs:
        assert chans.setdefault(int(r["index"]), channel(r["flags"])) == channel(r["flags"]), "a cut changed its channel"
    return assemble(recs)
