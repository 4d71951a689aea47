// gate.hip -- the live speech gate (uvad_gate_*, include/uvad.h): per feed and per step, the samples of the speech cuts the step's new
// labels and samples decide, as fragments with records.  The streaming counterpart of cuts.hip's table + gather: a session's fragments,
// concatenated per cut, are the bytes uvad_cuts_table + uvad_cuts_gather(UVAD_CUTS_SAMPLES) give on the whole session.
//
// One workgroup of GATE_THREADS per slot, three phases with a barrier between them:
//   1 commit   all lanes copy the slot's chunk row into its ring at the write position (two spans when it crosses the ring's end);
//   2 walk     gate_walk.h's interval machine: the labels come into LDS GATE_LAB_TILE at a time (the first round is fetched before
//              phase 1, so that its misses fly with the chunk's) and lane 0 walks them; every piece that closes, and at the end the piece
//              still open, becomes one record, stored to d_seg as it is made.  Lane 0 then writes the slot back and the count;
//   3 copy     all lanes read the records back (the barrier orders lane 0's stores before them) and copy fragment after fragment
//              from the ring to the output row (gate_walk.h's gate_copy_fragment).
// The walk, the span copy and the fragment copy are shared with gate_group.hip; this file holds what is the mono gate's own: the slot,
// the one ring per slot and the launch.  No atomics; an idle slot reads no input and writes only its count.
//   launch_gate_reset   the header (magic, B, the uvad_cuts_cfg, unit size, ring length) by field name, through launch_state_reset, which
//                       also leaves every slot idle; the rings are not touched: a session reads only what it has written
//   gate_step_kernel    the step above
#include <cstddef>
#include "gate_walk.h"

namespace uvad {

static_assert(sizeof(GateHeader) == 256 && sizeof(GateSlot) == 64 && sizeof(GateSeg) == 32 && sizeof(uvad_gate_seg) == 32, "uvad_gate state and record");
static_assert(offsetof(uvad_gate_seg, offset) == offsetof(GateSeg, offset) && offsetof(uvad_gate_seg, n_stored) == offsetof(GateSeg, n_stored), "uvad_gate_seg");
static_assert(UVAD_GATE_FIRST == 1 && UVAD_GATE_LAST == 2 && UVAD_GATE_LOST == 4 && UVAD_GATE_SHORT == 8, "record flags");

namespace {

template <class G> __global__ __launch_bounds__(GATE_THREADS) void gate_step_kernel(GateArgs a) {
    __shared__ uint8_t tile[GATE_LAB_TILE];
    __shared__ int sh_nrec;
    const GateHeader *hd = reinterpret_cast<const GateHeader *>(a.state);
    const int b = blockIdx.x, tid = threadIdx.x;
    if (hd->magic != GATE_MAGIC || hd->B != a.B || b >= a.B || hd->unit_bytes != (int)sizeof(G)) return;   // not the state this launch was sized for
    const long long P = hd->q.pad, W = hd->q.max_len, hop = hd->q.hop, lead = hd->q.lead, tl = hd->q.tail, H = hd->history;
    if (P < 0 || P > CUTS_MAX_PAD || W < 0 || W > CUTS_MAX_LEN || hop < 1 || lead < 0 || tl < 0 || H < a.chunk_n || a.chunk_n < 1 ||
        hd->ring_bytes != (long long)gate_ring_bytes((int)sizeof(G), H))
        return;
    char *base = reinterpret_cast<char *>(a.state) + sizeof(GateHeader);
    GateSlot *S = reinterpret_cast<GateSlot *>(base) + b;
    G *ring = reinterpret_cast<G *>(base + (size_t)a.B * sizeof(GateSlot) + (size_t)b * (size_t)hd->ring_bytes);

    const int fl = a.flags ? a.flags[b] : 0;
    GateSlot st = *S;                                                       // every lane holds the slot as the step found it
    if (fl & UVAD_SLOT_START) {                                             // the old session is dropped silently; the ring runs on
        const int wp = st.wp;
        st = GateSlot{};
        st.wp = wp;
        st.live = 1;
    }
    if (!st.live) {                                                         // idle: no input is read
        if (tid == 0) a.seg_counts[b] = 0;
        return;
    }
    int wp = st.wp;
    wp = wp < 0 || wp >= H ? 0 : wp;
    int nb = 0;
    if (a.ld_lab > 0) {
        nb = a.lab_counts[b];
        nb = nb < 0 ? 0 : nb > a.ld_lab ? a.ld_lab : nb;
    }
    const uint8_t *lab = a.labels + (size_t)b * a.ld_lab;
    // the first round of labels is fetched here, so that its misses fly with the chunk's; columns past the count are never read
    for (int i = tid; i < nb && i < GATE_LAB_TILE; i += GATE_THREADS) tile[i] = lab[i];

    // 1 commit the chunk, then read
    {
        const G *row = reinterpret_cast<const G *>(a.chunk) + (size_t)b * a.chunk_n;
        const long long n1 = a.chunk_n < H - wp ? a.chunk_n : H - wp;
        gate_copy_span(ring + wp, row, n1, tid);
        gate_copy_span(ring, row + n1, a.chunk_n - n1, tid);
        wp = (int)((wp + (long long)a.chunk_n) % H);
    }
    const long long A = st.A + a.chunk_n;
    const bool ending = (fl & UVAD_SLOT_END) != 0;
    GateSeg *seg = (a.seg && a.max_seg > 0) ? a.seg + (size_t)b * a.max_seg : nullptr;
    const long long room = a.out ? a.ld_out : 0;

    // 2 the walk: lane 0's result is the slot
    GateWalkCfg wq{};
    wq.P = P; wq.W = W; wq.hop = hop; wq.lead = lead; wq.tail = tl; wq.A = A; wq.H = H; wq.room = room; wq.ending = ending; wq.seg = seg;
    wq.max_seg = a.max_seg;
    GateWalkSlot ws{};
    ws.sent = st.sent; ws.pf = st.pf; ws.c = st.c; ws.F = st.F; ws.idx = st.idx; ws.mode = st.mode; ws.started = st.started;
    __syncthreads();                                                        // the chunk is in the ring, the first labels in LDS
    ws = gate_walk<false>(wq, ws, tile, lab, nb, tid);
    if (tid == 0) {
        GateSlot o{};
        o.wp = wp;
        if (!ending) {
            o.A = A; o.sent = ws.sent; o.F = (int)ws.F; o.c = (int)ws.c; o.pf = (int)ws.pf; o.idx = ws.idx; o.mode = ws.mode; o.started = ws.started;
            o.live = 1;
        }
        *S = o;
        a.seg_counts[b] = ws.nrec;
        sh_nrec = ws.nrec < a.max_seg ? ws.nrec : a.max_seg;
    }
    __syncthreads();                                                        // lane 0's records are visible to the workgroup

    // 3 the copy
    if (!seg) return;
    const int lim = sh_nrec;
    G *orow = reinterpret_cast<G *>(a.out) + (size_t)b * (size_t)a.ld_out;
    long long off = 0;
    for (int r = 0; r < lim; ++r) {
        const GateSeg q = seg[r];
        if (q.n_stored <= 0) continue;
        gate_copy_fragment(orow + off, ring, q, A, H, wp, hop, lead, tid);
        off += q.n_stored;
    }
}

}  // namespace

hipError_t launch_gate_reset(void *state, int B, const CutsCfgInt &q, int unit_bytes, int history, hipStream_t s) {
    if (!state || B <= 0 || (unit_bytes != 2 && unit_bytes != 4) || history < 1) return hipErrorInvalidValue;
    GateHeader h{};
    h.magic = GATE_MAGIC; h.B = B; h.q = q; h.unit_bytes = unit_bytes; h.history = history;
    h.ring_bytes = (long long)gate_ring_bytes(unit_bytes, history);
    return launch_state_reset(state, header_words(h), (long long)((sizeof(GateHeader) + (size_t)B * sizeof(GateSlot)) / sizeof(unsigned)), s);
}

hipError_t launch_gate_step(const GateArgs &a, int unit_bytes, hipStream_t s) {
    if (!a.chunk || !a.state || !a.seg_counts || a.B <= 0 || a.chunk_n < 1 || a.chunk_n > GATE_MAX_CHUNK || a.ld_lab < 0 ||
        (a.ld_lab > 0 && (!a.labels || !a.lab_counts)) || a.ld_out < 0 || (a.ld_out > 0 && !a.out) || a.max_seg < 0 || (a.max_seg > 0 && !a.seg) ||
        (unit_bytes != 2 && unit_bytes != 4))
        return hipErrorInvalidValue;
    if (unit_bytes == 2) hipLaunchKernelGGL(gate_step_kernel<uint16_t>, dim3((unsigned)a.B), dim3(GATE_THREADS), 0, s, a);
    else hipLaunchKernelGGL(gate_step_kernel<uint32_t>, dim3((unsigned)a.B), dim3(GATE_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
