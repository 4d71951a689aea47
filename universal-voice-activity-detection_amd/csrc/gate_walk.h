// gate_walk.h -- what the two live speech gates share on the device (gate.hip, gate_group.hip; device code only): the copy of a span, the
// copy of a record's fragment out of a ring, and the interval machine that walks a step's labels and makes the step's records.  One
// workgroup of GATE_THREADS lanes calls each of them.  The cut rule (pad, max_len, tail, SHORT, LOST) lives here and nowhere else.
#pragma once
#include <climits>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

// n units from src (nullptr: zeros) to dst, by all lanes of the workgroup; dst and src are unit-aligned, nothing more is assumed.
// 16 bytes per lane between the destination's first and last 16-byte boundary -- one 16-byte load when the source happens to be aligned
// there too, loads of the unit's own size otherwise -- and unit by unit at the two edges.
template <class U> __device__ __forceinline__ void gate_copy_span(U *dst, const U *src, long long n, int tid) {
    constexpr int V = 16 / (int)sizeof(U);
    if (n <= 0) return;
    long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(U));
    head = head < n ? head : n;
    const long long body = (n - head) / V, tail0 = head + body * V;
    for (long long i = tid; i < head; i += GATE_THREADS) dst[i] = src ? src[i] : (U)0;
    U *d = dst + head;
    const U *s = src ? src + head : nullptr;
    const bool same = s && (reinterpret_cast<uintptr_t>(s) & 15u) == 0;
    for (long long v = tid; v < body; v += GATE_THREADS) {
        union { U e[V]; uint4 q; } u;
        if (same) {
            u.q = *reinterpret_cast<const uint4 *>(s + v * V);
        } else if (s) {
#pragma unroll
            for (int k = 0; k < V; ++k) u.e[k] = s[v * V + k];
        } else {
            u.q = make_uint4(0u, 0u, 0u, 0u);
        }
        *reinterpret_cast<uint4 *>(d + v * V) = u.q;
    }
    for (long long i = tail0 + tid; i < n; i += GATE_THREADS) dst[i] = src ? src[i] : (U)0;
}

// the n_stored > 0 samples of record q from `ring` (H units, write position wp after a session total of A samples) to dst, by all lanes:
// zeros for the samples that have left the ring, then at most two spans of it
template <class U>
__device__ __forceinline__ void gate_copy_fragment(U *dst, const U *ring, const GateSeg &q, long long A, long long H, int wp, long long hop,
                                                   long long lead, int tid) {
    const long long ns = q.n_stored;
    long long first = (long long)q.first_frame * hop - lead;
    first = first < 0 ? 0 : first;
    const long long p0 = first + q.offset;                                  // the fragment is samples [p0, p0 + ns) of the session, p0 + ns <= A
    long long gone = A - H - p0;                                            // samples that have left the ring: zeros
    gone = gone < 0 ? 0 : gone > ns ? ns : gone;
    gate_copy_span<U>(dst, nullptr, gone, tid);
    const long long m = ns - gone, back = A - (p0 + gone);                  // sample p sits A - p places behind the write position
    if (m > 0 && back >= m && back <= H) {
        long long at = wp - back;
        at = at < 0 ? at + H : at;
        const long long m1 = m < H - at ? m : H - at;
        gate_copy_span(dst + gone, ring + at, m1, tid);
        gate_copy_span(dst + gone + m1, ring, m - m1, tid);
    }
}

// what a step's walk is given besides the slot: the header's cut rule, the session's samples after this step's chunk (A) and the ring's
// length (H), the step's record row (seg, max_seg; room = samples of its output row) and whether the session ends with this step.
// GROUP only: D, the decision horizon; ch0, the channel of the piece the step found started; unsync, the session's lockstep mark.
struct GateWalkCfg {
    long long P, W, hop, lead, tail, A, H, D, room;
    bool ending;
    GateSeg *seg;
    int max_seg, ch0, unsync;
};
// the interval machine's part of a slot (GateSlot's fields of these names), in and out; out only: nrec, the step's records (stored or
// not), and GROUP only: open_f / open_w, the first frame and the number of deciding frames of a piece whose first record was made in
// this step and which stays open (open_w = 0: none), and cont, 1 while the current piece is still the one the step found started
struct GateWalkSlot {
    long long sent, pf, c, F;
    int idx, mode, started;
    int nrec, open_w, cont;
    long long open_f;
};

// Phase 2 of both step kernels, called by the whole workgroup once the first GATE_LAB_TILE labels of lab[0 .. nb) are in `tile` and a
// barrier has passed: the labels come into LDS a tile at a time (all lanes) and lane 0 walks them one by one -- IDLE / inside a run /
// PENDING after a run, the current piece's first frame, its index and the samples it has delivered.  Every piece that closes, and at
// the end of the step the piece still open, becomes one record, stored to q.seg as it is made.  Only lane 0's return value is the slot.
// The working state is plain locals with lambdas over them, copied in and out: held as a struct it does not stay in registers.
// GROUP (gate_group.hip) differs in four places, all in record / close below:
//   - a piece without a record that stays open gives none while fewer than D of its frames are known (its channel is not final);
//   - a FIRST record carries no channel and is noted in open_f / open_w if the piece stays open: the kernel's pick phase patches it in;
//   - a later record of the piece the step found started carries ch0 in bits 8 .. 15, and every record UNSYNC if the session is marked;
//   - cont tells the kernel whether the slot keeps ch0.
template <bool GROUP>
__device__ __forceinline__ GateWalkSlot gate_walk(const GateWalkCfg &q, const GateWalkSlot in, uint8_t *tile, const uint8_t *lab, int nb, int tid) {
    const long long P = q.P, W = q.W, hop = q.hop, lead = q.lead, tl = q.tail, A = q.A, H = q.H, D = q.D, room = q.room;
    const bool ending = q.ending;
    GateSeg *seg = q.seg;
    long long sent = in.sent, pf = in.pf, c = in.c, F = in.F, out_off = 0, open_f = 0;
    int idx = in.idx, mode = in.mode, started = in.started, nrec = 0, open_w = 0, cont = in.started;
    // the current piece, k frames so far, delivers its samples up to the absolute position upto
    auto record = [&](int flags, long long k, long long upto) {
        if (GROUP && !started && !(flags & UVAD_GATE_LAST) && k < D) return;   // deferred: the first `decide` frames are not all known yet
        long long first = pf * hop - lead;
        first = first < 0 ? 0 : first;
        long long total = upto - first;
        total = total < 0 ? 0 : total;
        long long n = total - sent;
        n = n < 0 ? 0 : n;
        if (!(flags & UVAD_GATE_LAST) && n == 0) return;                    // an open piece with nothing new says nothing
        const long long src = first + sent;
        if (!started) {
            flags |= UVAD_GATE_FIRST;                                       // GROUP: the pick phase chooses the channel and patches it in
            if (GROUP && !(flags & UVAD_GATE_LAST)) { open_f = pf; open_w = (int)(k < D ? k : D); }
        } else if (GROUP) {
            flags |= q.ch0 << 8;                                            // a piece has one record per step: this one started in an earlier step
        }
        if (GROUP && q.unsync) flags |= GATE_GROUP_UNSYNC;
        if (n > 0 && src < A - H) flags |= UVAD_GATE_LOST;
        if (seg && nrec < q.max_seg) {
            const long long n32 = n > INT_MAX ? INT_MAX : n, left = room - out_off;
            const long long ns = n32 < left ? n32 : left;
            GateSeg r;
            r.index = idx; r.flags = flags; r.first_frame = (int)pf; r.n_frames = (int)k; r.offset = sent; r.n = (int)n32; r.n_stored = (int)ns;
            seg[nrec] = r;
            out_off += ns;
        }
        if (nrec < INT_MAX) ++nrec;
        sent = total;
        started = 1;
    };
    auto close = [&](long long k) {                                         // the current piece closes with k frames
        const long long want = (pf + k) * hop + tl;
        record(UVAD_GATE_LAST | ((!ending && A < want) ? UVAD_GATE_SHORT : 0), k, want < A ? want : A);
        if (idx < INT_MAX) ++idx;
        pf += k;
        sent = 0;
        started = 0;
        if (GROUP) { cont = 0; open_w = 0; }
    };
    auto cover = [&](long long g) {                                         // frames below g are known to lie inside the interval
        while (W && g - pf >= W) close(W);
    };
    auto known = [&]() { return mode == EP_SPEECH ? F : (c + P < F ? c + P : F); };

    for (int t0 = 0; t0 < nb; t0 += GATE_LAB_TILE) {
        const int cnt = nb - t0 < GATE_LAB_TILE ? nb - t0 : GATE_LAB_TILE;
        if (t0 > 0) {
            for (int i = tid; i < cnt; i += GATE_THREADS) tile[i] = lab[t0 + i];
            __syncthreads();
        }
        if (tid == 0) {
            for (int i = 0; i < cnt && F < INT_MAX; ++i) {
                const bool v = tile[i] != 0;
                const long long t = F;
                if (mode == EP_IDLE && v) {
                    pf = t > P ? t - P : 0;
                    mode = EP_SPEECH;
                } else if (mode == EP_SPEECH && !v) {
                    c = t;
                    mode = EP_PENDING;
                } else if (mode == EP_PENDING && v) {
                    mode = EP_SPEECH;                                       // the run rejoins
                }
                F = t + 1;
                if (mode == EP_PENDING && !v && t >= c + 2 * P) {
                    const long long hi = c + P;
                    cover(hi);
                    if (hi > pf) close(hi - pf);
                    mode = EP_IDLE;
                } else if (mode != EP_IDLE) {
                    cover(known());
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0 && mode != EP_IDLE) {                                      // the end of the step: the piece still open
        const long long g = known();
        if (ending) {
            cover(g);
            if (g > pf) close(g - pf);
        } else if (g > pf) {
            const long long upto = g * hop < A ? g * hop : A;
            record(0, g - pf, upto);
        }
    }
    GateWalkSlot o;
    o.sent = sent; o.pf = pf; o.c = c; o.F = F; o.idx = idx; o.mode = mode; o.started = started;
    o.nrec = nrec; o.open_w = open_w; o.cont = cont; o.open_f = open_f;
    return o;
}

}  // namespace uvad
