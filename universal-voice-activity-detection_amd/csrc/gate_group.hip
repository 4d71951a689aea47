// gate_group.hip -- the live speech gate for fused groups (uvad_gate_group_*, include/uvad.h): per group of the fusion configuration and
// per step, the samples of the group's speech cuts, each cut taken whole from ONE member channel: the member that won most of the cut's
// first `decide` frames in uvad_fuse's d_best.  The streaming counterpart of uvad_cuts_table + uvad_fuse_pick + uvad_cuts_gather, as
// gate.hip is of the table + gather.  The interval machine, the span copy and the fragment copy are gate_walk.h's, shared with gate.hip;
// gate_walk<true> differs from the mono gate's walk in four places, all of them about the channel:
//   - deferral: a piece whose channel is not final -- it has no record yet, it stays open and fewer than `decide` of its frames are known
//     to lie inside the interval -- gives no record, so the first record of a piece carries its whole backlog;
//   - flag bits: that first record is the one place where a channel is chosen: it is stored with UVAD_GATE_FIRST and without a channel;
//     a later record of the piece the step found started carries the slot's channel in bits 8 .. 15, and every record of a session whose
//     members fell out of lockstep carries UVAD_GATE_UNSYNC;
//   - open_f / open_w: the walk reports the piece that got its first record in this step and stays open, so that phase 3 picks for it;
//   - cont: the walk reports whether the piece the step found started is still the current one, i.e. whether the slot keeps its channel.
//
// One workgroup of GATE_THREADS per group, four phases with a barrier between them:
//   1 commit   all lanes copy every member's chunk row into that member slot's ring (all rings of a group share the write position) and
//              the step's best bytes into the group's best ring;
//   2 walk     gate_walk<true>: the labels come into LDS GATE_LAB_TILE at a time and lane 0 walks them; lane 0 then writes the slot back;
//   3 pick     one wave per FIRST record: the best ring's bytes of frames [f, f + min(k, decide)) go by 64 at a time, one ballot per
//              member position present among the 64, lane k holds the count of positions k, k + 64, ...; a shuffle tree takes the largest
//              count, ties to the lowest position (fuse.hip's pick).  Frames at or past the best bytes received, or out of the ring, vote
//              for nobody.  Lane 0 patches the position into bits 8 .. 15 of the record's flags; the pick of the piece still open goes
//              into the slot, from which later steps' records of that piece take it;
//   4 copy     all lanes copy fragment after fragment from the chosen member's ring (gate_copy_fragment).
// Every ring index is reduced modulo the header's lengths and every store is bounded by ld_out / max_seg whatever the state holds; a
// header that is not this launch's makes the launch touch nothing.  No atomics; an idle group reads no input and writes only its count.
//   launch_gate_group_reset   the header by field name, through launch_state_reset, which also leaves every group idle; no ring is touched
#include <cstddef>
#include "gate_walk.h"

namespace uvad {

static_assert(sizeof(GateGroupHeader) == 256 && sizeof(GateGroupSlot) == 96 && sizeof(GateSeg) == sizeof(uvad_gate_seg), "uvad_gate_group state");
static_assert(UVAD_GATE_UNSYNC == GATE_GROUP_UNSYNC && UVAD_GATE_CHANNEL(0x1234) == 0x12 && FUSE_MAX_MEMBERS <= 255, "record flags");

namespace {

typedef unsigned long long u64;

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

template <class U> __global__ __launch_bounds__(GATE_THREADS) void gate_group_step_kernel(GateGroupArgs a) {
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
    for (int i = tid; i < nb && i < GATE_LAB_TILE; i += GATE_THREADS) tile[i] = lab[i];

    // 1 commit the members' chunks and the best bytes, then read
    for (int j = 0; j < M; ++j) {
        const U *row = reinterpret_cast<const U *>(a.chunk) + (size_t)a.members[j0 + j] * a.chunk_n;
        U *ring = ring_of(j);
        const long long n1 = a.chunk_n < H - wp ? a.chunk_n : H - wp;
        gate_copy_span(ring + wp, row, n1, tid);
        gate_copy_span(ring, row + n1, a.chunk_n - n1, tid);
    }
    wp = (int)((wp + (long long)a.chunk_n) % H);
    {
        const uint8_t *brow = a.best + (size_t)g * a.ld_best;
        const long long skip = nbest > BH ? nbest - BH : 0;                 // more than the ring holds: only the last BH stay
        for (long long i = skip + tid; i < nbest; i += GATE_THREADS) bring[(bwp + i) % BH] = brow[i];
        bwp = (int)((bwp + (long long)nbest) % BH);
    }
    const long long A = st.A + a.chunk_n, Fb = st.Fb + nbest;
    const bool ending = (fl & UVAD_SLOT_END) != 0;
    GateSeg *seg = (a.seg && a.max_seg > 0) ? a.seg + (size_t)g * a.max_seg : nullptr;
    const long long room = a.out ? a.ld_out : 0;
    const int ch0 = (unsigned)st.ch < (unsigned)M ? st.ch : 0;              // the channel of the piece the step found started

    // 2 the walk: lane 0's result is the slot
    GateWalkCfg wq{};
    wq.P = P; wq.W = W; wq.hop = hop; wq.lead = lead; wq.tail = tl; wq.A = A; wq.H = H; wq.D = D; wq.room = room; wq.ending = ending; wq.seg = seg;
    wq.max_seg = a.max_seg; wq.ch0 = ch0; wq.unsync = unsync;
    GateWalkSlot ws{};
    ws.sent = st.sent; ws.pf = st.pf; ws.c = st.c; ws.F = st.F; ws.idx = st.idx; ws.mode = st.mode; ws.started = st.started;
    __syncthreads();                                                        // the chunks and best bytes are in the rings, the first labels in LDS
    ws = gate_walk<true>(wq, ws, tile, lab, nb, tid);
    if (tid == 0) {
        GateGroupSlot o{};
        o.wp = wp; o.bwp = bwp;
        if (!ending) {
            o.A = A; o.sent = ws.sent; o.Fb = Fb; o.F = (int)ws.F; o.c = (int)ws.c; o.pf = (int)ws.pf; o.idx = ws.idx; o.mode = ws.mode;
            o.started = ws.started; o.live = 1;
            o.ch = ws.cont ? ch0 : 0;                                       // a piece that started in this step: phase 3 writes its channel
            o.unsync = unsync;
        }
        *S = o;
        a.seg_counts[g] = ws.nrec;
        sh_nrec = ws.nrec < a.max_seg ? ws.nrec : a.max_seg;
        sh_open_w = ending ? 0 : ws.open_w;
        sh_open_f = ws.open_f;
    }
    __syncthreads();                                                        // lane 0's records and the slot are visible to the workgroup

    // 3 the picks: one wave per FIRST record, and wave 0 for the piece that stays open
    const int lim = seg ? sh_nrec : 0;
    for (int r = wave; r < lim; r += GATE_THREADS / 64) {
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
        if (q.n_stored <= 0) continue;
        int pos = UVAD_GATE_CHANNEL(q.flags);
        pos = pos < M ? pos : 0;
        gate_copy_fragment(orow + off, ring_of(pos), q, A, H, wp, hop, lead, tid);
        off += q.n_stored;
    }
}

}  // namespace

hipError_t launch_gate_group_reset(void *state, int G, int N, const CutsCfgInt &q, int unit_bytes, int history, int best_history, int decide,
                                   hipStream_t s) {
    if (!state || G <= 0 || N < G || (unit_bytes != 2 && unit_bytes != 4) || history < 1 || best_history < 1 || decide < 1) return hipErrorInvalidValue;
    GateGroupHeader h{};
    h.magic = GATE_GROUP_MAGIC; h.G = G; h.N = N; h.q = q; h.unit_bytes = unit_bytes; h.history = history; h.best_history = best_history;
    h.decide = decide; h.ring_bytes = (long long)gate_ring_bytes(unit_bytes, history); h.best_bytes = (long long)gate_group_best_bytes(best_history);
    return launch_state_reset(state, header_words(h), (long long)((sizeof(GateGroupHeader) + (size_t)G * sizeof(GateGroupSlot)) / sizeof(unsigned)), s);
}

hipError_t launch_gate_group_step(const GateGroupArgs &a, int unit_bytes, hipStream_t s) {
    if (!a.first || !a.members || !a.chunk || !a.state || !a.seg_counts || a.G <= 0 || a.N < a.G || a.B <= 0 || a.chunk_n < 1 || a.chunk_n > GATE_MAX_CHUNK ||
        a.ld_lab < 0 || (a.ld_lab > 0 && (!a.labels || !a.lab_counts)) || a.ld_best < 0 || (a.ld_best > 0 && (!a.best || !a.best_counts)) || a.ld_out < 0 ||
        (a.ld_out > 0 && !a.out) || a.max_seg < 0 || (a.max_seg > 0 && !a.seg) || (unit_bytes != 2 && unit_bytes != 4))
        return hipErrorInvalidValue;
    if (unit_bytes == 2) hipLaunchKernelGGL(gate_group_step_kernel<uint16_t>, dim3((unsigned)a.G), dim3(GATE_THREADS), 0, s, a);
    else hipLaunchKernelGGL(gate_group_step_kernel<uint32_t>, dim3((unsigned)a.G), dim3(GATE_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
