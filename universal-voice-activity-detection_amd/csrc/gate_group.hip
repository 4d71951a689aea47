// gate_group.hip -- the live speech gate for fused groups (uvad_gate_group_*, include/uvad.h): per group of the fusion configuration and
// per step, the samples of the group's speech cuts, each cut taken whole from ONE member channel: the member that won most of the cut's
// first `decide` frames in uvad_fuse's d_best.  The streaming counterpart of uvad_cuts_table + uvad_fuse_pick + uvad_cuts_gather, as
// gate.hip is of the table + gather; the walk below is gate.hip's with one change: a piece gives no record until its channel is final.
//
// One workgroup of GATE_GROUP_THREADS per group, four phases with a barrier between them:
//   1 commit   all lanes copy every member's chunk row into that member slot's ring (all rings of a group share the write position) and
//              the step's best bytes into the group's best ring;
//   2 walk     the labels come into LDS GATE_LAB_TILE at a time and lane 0 walks them with the interval machine of gate.hip.  A piece
//              whose channel is not final -- it has no record yet, it stays open and fewer than `decide` of its frames are known to lie
//              inside the interval -- gives no record; the first record of a piece therefore carries its whole backlog, and is the one
//              place where a channel is chosen: it is stored with UVAD_GATE_FIRST and without a channel;
//   3 pick     one wave per FIRST record: the best ring's bytes of frames [f, f + min(k, decide)) go by 64 at a time, one ballot per
//              member position present among the 64, lane k holds the count of positions k, k + 64, ...; a shuffle tree takes the largest
//              count, ties to the lowest position (fuse.hip's pick).  Frames at or past the best bytes received, or out of the ring, vote
//              for nobody.  Lane 0 patches the position into bits 8 .. 15 of the record's flags; the pick of the piece still open goes
//              into the slot, from which later steps' records of that piece take it;
//   4 copy     all lanes copy fragment after fragment from the chosen member's ring: zeros for samples that have left it, then at most
//              two spans, 16 bytes per lane between the destination's 16-byte boundaries and unit by unit at the edges (gate.hip's copy).
// Every ring index is reduced modulo the header's lengths and every store is bounded by ld_out / max_seg whatever the state holds; a
// header that is not this launch's makes the launch touch nothing.  No atomics; an idle group reads no input and writes only its count.
#include <climits>
#include <cstddef>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

static_assert(sizeof(GateGroupHeader) == 256 && sizeof(GateGroupSlot) == 96 && sizeof(GateSeg) == sizeof(uvad_gate_seg), "uvad_gate_group state");
static_assert(UVAD_GATE_UNSYNC == GATE_GROUP_UNSYNC && UVAD_GATE_CHANNEL(0x1234) == 0x12 && FUSE_MAX_MEMBERS <= 255, "record flags");

namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void gate_group_reset_kernel(unsigned *state, int G, int N, CutsCfgInt q, int unit_bytes, int history, int best_history,
                                                               int decide) {
    const long long n = (long long)((sizeof(GateGroupHeader) + (size_t)G * sizeof(GateGroupSlot)) / sizeof(unsigned));
    const u64 rb = gate_ring_bytes(unit_bytes, history), bb = gate_group_best_bytes(best_history);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        unsigned v = 0u;
        if (i == 0) v = GATE_GROUP_MAGIC;
        else if (i == 1) v = (unsigned)G;
        else if (i == 2) v = (unsigned)N;
        else if (i == 3) v = (unsigned)q.pad;
        else if (i == 4) v = (unsigned)q.max_len;
        else if (i == 5) v = (unsigned)q.min_len;
        else if (i == 6) v = (unsigned)q.hop;
        else if (i == 7) v = (unsigned)q.lead;
        else if (i == 8) v = (unsigned)q.tail;
        else if (i == 9) v = (unsigned)unit_bytes;
        else if (i == 10) v = (unsigned)history;
        else if (i == 11) v = (unsigned)best_history;
        else if (i == 12) v = (unsigned)decide;
        else if (i == 14) v = (unsigned)(rb & 0xffffffffull);
        else if (i == 15) v = (unsigned)(rb >> 32);
        else if (i == 16) v = (unsigned)(bb & 0xffffffffull);
        else if (i == 17) v = (unsigned)(bb >> 32);
        state[i] = v;
    }
}

// n units from src (nullptr: zeros) to dst, by all lanes of the workgroup; dst and src are unit-aligned, nothing more is assumed
template <class U> __device__ __forceinline__ void gg_copy_span(U *dst, const U *src, long long n, int tid) {
    constexpr int V = 16 / (int)sizeof(U);
    if (n <= 0) return;
    long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(U));
    head = head < n ? head : n;
    const long long body = (n - head) / V, tail0 = head + body * V;
    for (long long i = tid; i < head; i += GATE_GROUP_THREADS) dst[i] = src ? src[i] : (U)0;
    U *d = dst + head;
    const U *s = src ? src + head : nullptr;
    const bool same = s && (reinterpret_cast<uintptr_t>(s) & 15u) == 0;
    for (long long v = tid; v < body; v += GATE_GROUP_THREADS) {
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
    for (long long i = tail0 + tid; i < n; i += GATE_GROUP_THREADS) dst[i] = src ? src[i] : (U)0;
}

// by one whole wave: the member position (0 .. M - 1) with the most frames t of [f, f + w) whose best byte, read from the ring, equals
// it; ties to the lowest position, no votes: position 0.  Fb best bytes have been received and the ring's write position is bwp: frame
// t sits Fb - t places behind it; frames at or past Fb, or more than BH behind, vote for nobody.  Every lane returns the same value.
__device__ __forceinline__ int gg_pick(const uint8_t *bring, long long BH, long long bwp, long long Fb, long long f, long long w, int M, int lane) {
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;                           // lane k: the frames won by positions k, k + 64, k + 128, k + 192
    for (long long f0 = f; f0 < f + w; f0 += 64) {
        const long long t = f0 + lane, back = Fb - t;
        int b = -1;
        if (t < f + w && t >= 0 && back >= 1 && back <= BH) {
            long long at = bwp - back;
            at = at < 0 ? at + BH : at;
            b = (int)bring[at];
        }
        u64 rem = (u64)__ballot(b >= 0);
        while (rem) {                                            // one ballot per position present among the 64
            const int v = __shfl(b, __ffsll((long long)rem) - 1);
            const u64 hit = (u64)__ballot(b == v);
            const int c = __popcll(hit);
            if (lane == (v & 63)) {
                const int q = v >> 6;
                c0 += q == 0 ? c : 0; c1 += q == 1 ? c : 0; c2 += q == 2 ? c : 0; c3 += q == 3 ? c : 0;
            }
            rem &= ~hit;
        }
    }
    int bc = -1, bp = 0x7fffffff;
    if (lane < M) { bc = c0; bp = lane; }
    if (lane + 64 < M && c1 > bc) { bc = c1; bp = lane + 64; }
    if (lane + 128 < M && c2 > bc) { bc = c2; bp = lane + 128; }
    if (lane + 192 < M && c3 > bc) { bc = c3; bp = lane + 192; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_down(bc, o), op = __shfl_down(bp, o);
        if (oc > bc || (oc == bc && op < bp)) { bc = oc; bp = op; }
    }
    return __shfl(bp, 0);                                        // M >= 1: position 0 always stands
}

template <class U> __global__ __launch_bounds__(GATE_GROUP_THREADS) void gate_group_step_kernel(GateGroupArgs a) {
    __shared__ uint8_t tile[GATE_LAB_TILE];
    __shared__ int sh_nrec, sh_open_w;
    __shared__ long long sh_open_f;
    const GateGroupHeader *hd = reinterpret_cast<const GateGroupHeader *>(a.state);
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (hd->magic != GATE_GROUP_MAGIC || hd->G != a.G || hd->N != a.N || g >= a.G || hd->unit_bytes != (int)sizeof(U)) return;   // not this launch's state
    const long long P = hd->q.pad, W = hd->q.max_len, hop = hd->q.hop, lead = hd->q.lead, tl = hd->q.tail, H = hd->history, BH = hd->best_history,
                    D = hd->decide;
    if (P < 0 || P > CUTS_MAX_PAD || W < 0 || W > CUTS_MAX_LEN || hop < 1 || lead < 0 || tl < 0 || H < a.chunk_n || a.chunk_n < 1 || BH < 1 || D < 1 ||
        D > CUTS_MAX_LEN || hd->ring_bytes != (long long)gate_ring_bytes((int)sizeof(U), H) || hd->best_bytes != (long long)gate_group_best_bytes(BH))
        return;
    const int j0 = a.first[g], M = a.first[g + 1] - j0;             // 1 .. 255 and inside N, checked at configure; checked again: they index the state
    if (j0 < 0 || M < 1 || M > FUSE_MAX_MEMBERS || j0 + M > a.N) return;
    char *base = reinterpret_cast<char *>(a.state) + sizeof(GateGroupHeader);
    GateGroupSlot *S = reinterpret_cast<GateGroupSlot *>(base) + g;
    uint8_t *bring = reinterpret_cast<uint8_t *>(base + (size_t)a.G * sizeof(GateGroupSlot) + (size_t)g * (size_t)hd->best_bytes);
    char *rings = base + (size_t)a.G * (sizeof(GateGroupSlot) + (size_t)hd->best_bytes);
    auto ring_of = [&](int pos) { return reinterpret_cast<U *>(rings + (size_t)(j0 + pos) * (size_t)hd->ring_bytes); };

    const int fl = a.gflags ? a.gflags[g] : 0;
    GateGroupSlot st = *S;                                                  // every lane holds the slot as the step found it
    if (fl & UVAD_SLOT_START) {                                             // the old session is dropped silently; the rings run on
        const int wp0 = st.wp, bwp0 = st.bwp;
        st = GateGroupSlot{};
        st.wp = wp0; st.bwp = bwp0;
        st.live = 1;
    }
    if (!st.live) {                                                         // idle: no input is read
        if (tid == 0) a.seg_counts[g] = 0;
        return;
    }
    // the lockstep check: the members' flag bytes of this step agree, or the session is marked from here to its END
    int differ = 0;
    if (a.rflags && tid < M) differ = a.rflags[a.members[j0 + tid]] != a.rflags[a.members[j0]];
    const int unsync = (__syncthreads_or(differ) || st.unsync) ? 1 : 0;

    int wp = st.wp, bwp = st.bwp;
    wp = wp < 0 || wp >= H ? 0 : wp;
    bwp = bwp < 0 || bwp >= BH ? 0 : bwp;
    int nb = 0, nbest = 0;
    if (a.ld_lab > 0) {
        nb = a.lab_counts[g];
        nb = nb < 0 ? 0 : nb > a.ld_lab ? a.ld_lab : nb;
    }
    if (a.ld_best > 0) {
        nbest = a.best_counts[g];
        nbest = nbest < 0 ? 0 : nbest > a.ld_best ? a.ld_best : nbest;
    }
    const uint8_t *lab = a.labels + (size_t)g * a.ld_lab;
    // the first round of labels is fetched here, so that its misses fly with the chunks'; columns past the count are never read
    for (int i = tid; i < nb && i < GATE_LAB_TILE; i += GATE_GROUP_THREADS) tile[i] = lab[i];

    // 1 commit the members' chunks and the best bytes, then read
    for (int j = 0; j < M; ++j) {
        const U *row = reinterpret_cast<const U *>(a.chunk) + (size_t)a.members[j0 + j] * a.chunk_n;
        U *ring = ring_of(j);
        const long long n1 = a.chunk_n < H - wp ? a.chunk_n : H - wp;
        gg_copy_span(ring + wp, row, n1, tid);
        gg_copy_span(ring, row + n1, a.chunk_n - n1, tid);
    }
    wp = (int)((wp + (long long)a.chunk_n) % H);
    {
        const uint8_t *brow = a.best + (size_t)g * a.ld_best;
        const long long skip = nbest > BH ? nbest - BH : 0;                 // more than the ring holds: only the last BH stay
        for (long long i = skip + tid; i < nbest; i += GATE_GROUP_THREADS) bring[(bwp + i) % BH] = brow[i];
        bwp = (int)((bwp + (long long)nbest) % BH);
    }
    const long long A = st.A + a.chunk_n, Fb = st.Fb + nbest;
    const bool ending = (fl & UVAD_SLOT_END) != 0;
    GateSeg *seg = (a.seg && a.max_seg > 0) ? a.seg + (size_t)g * a.max_seg : nullptr;
    const long long room = a.out ? a.ld_out : 0;
    const int ch0 = (unsigned)st.ch < (unsigned)M ? st.ch : 0;              // the channel of the piece the step found started

    // 2 the walk: lane 0's variables below are the slot
    long long sent = st.sent, pf = st.pf, c = st.c, F = st.F, out_off = 0, open_f = 0;
    int idx = st.idx, mode = st.mode, started = st.started, nrec = 0, open_w = 0, cont = st.started;
    // the current piece, k frames so far, delivers its samples up to the absolute position upto -- once its channel is final
    auto record = [&](int flags, long long k, long long upto) {
        if (!started && !(flags & UVAD_GATE_LAST) && k < D) return;         // deferred: the first `decide` frames are not all known yet
        long long first = pf * hop - lead;
        first = first < 0 ? 0 : first;
        long long total = upto - first;
        total = total < 0 ? 0 : total;
        long long n = total - sent;
        n = n < 0 ? 0 : n;
        if (!(flags & UVAD_GATE_LAST) && n == 0) return;                    // an open piece with nothing new says nothing
        const long long src = first + sent;
        if (!started) {
            flags |= UVAD_GATE_FIRST;                                       // phase 3 chooses the channel and patches it in
            if (!(flags & UVAD_GATE_LAST)) { open_f = pf; open_w = (int)(k < D ? k : D); }
        } else {
            flags |= ch0 << 8;                                              // a piece has one record per step: this one started in an earlier step
        }
        if (unsync) flags |= GATE_GROUP_UNSYNC;
        if (n > 0 && src < A - H) flags |= UVAD_GATE_LOST;
        if (seg && nrec < a.max_seg) {
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
        cont = 0;
        open_w = 0;
    };
    auto cover = [&](long long gg) {                                        // frames below gg are known to lie inside the interval
        while (W && gg - pf >= W) close(W);
    };
    auto known = [&]() { return mode == EP_SPEECH ? F : (c + P < F ? c + P : F); };

    __syncthreads();                                                        // the chunks and best bytes are in the rings, the first labels in LDS
    for (int t0 = 0; t0 < nb; t0 += GATE_LAB_TILE) {
        const int cnt = nb - t0 < GATE_LAB_TILE ? nb - t0 : GATE_LAB_TILE;
        if (t0 > 0) {
            for (int i = tid; i < cnt; i += GATE_GROUP_THREADS) tile[i] = lab[t0 + i];
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
    if (tid == 0) {
        if (mode != EP_IDLE) {
            const long long gg = known();
            if (ending) {
                cover(gg);
                if (gg > pf) close(gg - pf);
            } else if (gg > pf) {
                const long long upto = gg * hop < A ? gg * hop : A;
                record(0, gg - pf, upto);
            }
        }
        GateGroupSlot o{};
        o.wp = wp; o.bwp = bwp;
        if (!ending) {
            o.A = A; o.sent = sent; o.Fb = Fb; o.F = (int)F; o.c = (int)c; o.pf = (int)pf; o.idx = idx; o.mode = mode; o.started = started; o.live = 1;
            o.ch = cont ? ch0 : 0;                                          // a piece that started in this step: phase 3 writes its channel
            o.unsync = unsync;
        }
        *S = o;
        a.seg_counts[g] = nrec;
        sh_nrec = nrec < a.max_seg ? nrec : a.max_seg;
        sh_open_w = ending ? 0 : open_w;
        sh_open_f = open_f;
    }
    __syncthreads();                                                        // lane 0's records and the slot are visible to the workgroup

    // 3 the picks: one wave per FIRST record, and wave 0 for the piece that stays open
    const int lim = seg ? sh_nrec : 0;
    for (int r = wave; r < lim; r += GATE_GROUP_THREADS / 64) {
        const GateSeg q = seg[r];
        if (!(q.flags & UVAD_GATE_FIRST)) continue;
        const long long w = q.n_frames < D ? q.n_frames : D;
        const int p = gg_pick(bring, BH, bwp, Fb, q.first_frame, w, M, lane);
        if (lane == 0) seg[r].flags = q.flags | (p << 8);
    }
    if (wave == 0 && sh_open_w > 0) {
        const int p = gg_pick(bring, BH, bwp, Fb, sh_open_f, sh_open_w, M, lane);
        if (lane == 0) S->ch = p;
    }
    if (!seg) return;
    __syncthreads();                                                        // the channels are in the records

    // 4 the copy
    U *orow = reinterpret_cast<U *>(a.out) + (size_t)g * (size_t)a.ld_out;
    long long off = 0;
    for (int r = 0; r < lim; ++r) {
        const GateSeg q = seg[r];
        const long long ns = q.n_stored;
        if (ns <= 0) continue;
        int pos = UVAD_GATE_CHANNEL(q.flags);
        pos = pos < M ? pos : 0;
        const U *ring = ring_of(pos);
        long long first = (long long)q.first_frame * hop - lead;
        first = first < 0 ? 0 : first;
        const long long p0 = first + q.offset;                              // the fragment is samples [p0, p0 + ns) of the session, p0 + ns <= A
        long long gone = A - H - p0;                                        // samples that have left the ring: zeros
        gone = gone < 0 ? 0 : gone > ns ? ns : gone;
        U *dst = orow + off;
        gg_copy_span<U>(dst, nullptr, gone, tid);
        const long long m = ns - gone, back = A - (p0 + gone);              // sample p sits A - p places behind the write position
        if (m > 0 && back >= m && back <= H) {
            long long at = wp - back;
            at = at < 0 ? at + H : at;
            const long long m1 = m < H - at ? m : H - at;
            gg_copy_span(dst + gone, ring + at, m1, tid);
            gg_copy_span(dst + gone + m1, ring, m - m1, tid);
        }
        off += ns;
    }
}

}  // namespace

hipError_t launch_gate_group_reset(void *state, int G, int N, const CutsCfgInt &q, int unit_bytes, int history, int best_history, int decide,
                                   hipStream_t s) {
    if (!state || G <= 0 || N < G || (unit_bytes != 2 && unit_bytes != 4) || history < 1 || best_history < 1 || decide < 1) return hipErrorInvalidValue;
    const long long n = (long long)((sizeof(GateGroupHeader) + (size_t)G * sizeof(GateGroupSlot)) / sizeof(unsigned));
    const long long b = (n + 255) / 256;
    hipLaunchKernelGGL(gate_group_reset_kernel, dim3((unsigned)(b > 1024 ? 1024 : b)), dim3(256), 0, s, reinterpret_cast<unsigned *>(state), G, N, q,
                       unit_bytes, history, best_history, decide);
    return hipGetLastError();
}

hipError_t launch_gate_group_step(const GateGroupArgs &a, int unit_bytes, hipStream_t s) {
    if (!a.first || !a.members || !a.chunk || !a.state || !a.seg_counts || a.G <= 0 || a.N < a.G || a.B <= 0 || a.chunk_n < 1 || a.chunk_n > GATE_MAX_CHUNK ||
        a.ld_lab < 0 || (a.ld_lab > 0 && (!a.labels || !a.lab_counts)) || a.ld_best < 0 || (a.ld_best > 0 && (!a.best || !a.best_counts)) || a.ld_out < 0 ||
        (a.ld_out > 0 && !a.out) || a.max_seg < 0 || (a.max_seg > 0 && !a.seg) || (unit_bytes != 2 && unit_bytes != 4))
        return hipErrorInvalidValue;
    if (unit_bytes == 2) hipLaunchKernelGGL(gate_group_step_kernel<uint16_t>, dim3((unsigned)a.G), dim3(GATE_GROUP_THREADS), 0, s, a);
    else hipLaunchKernelGGL(gate_group_step_kernel<uint32_t>, dim3((unsigned)a.G), dim3(GATE_GROUP_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
