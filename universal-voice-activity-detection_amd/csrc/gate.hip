// gate.hip -- the live speech gate (uvad_gate_*, include/uvad.h): per feed and per step, the samples of the speech cuts the step's new
// labels and samples decide, as fragments with records.  The streaming counterpart of cuts.hip's table + gather: a session's fragments,
// concatenated per cut, are the bytes uvad_cuts_table + uvad_cuts_gather(UVAD_CUTS_SAMPLES) give on the whole session.
//
// One workgroup of GATE_THREADS per slot, three phases with a barrier between them:
//   1 commit   all lanes copy the slot's chunk row into its ring at the write position (two spans when it crosses the ring's end);
//   2 walk     the labels come into LDS GATE_LAB_TILE at a time (all lanes; the first round is fetched before phase 1, so that its
//              misses fly with the chunk's), and lane 0 walks them one by one with the slot's interval machine of the header: IDLE / inside a run / PENDING after a run, the current piece's first frame, its index and the
//              samples it has delivered.  Every piece that closes, and at the end the piece still open, becomes one record, stored to
//              d_seg as it is made: the step's fragment list.  Lane 0 then writes the slot back and the count;
//   3 copy     all lanes read the records back (the barrier orders lane 0's stores before them) and copy fragment after fragment
//              from the ring to the output row: zeros for samples that have left the ring, then at most two spans of the ring.
// A span is copied 16 bytes per lane between the destination's first and last 16-byte boundary -- one 16-byte load when the source
// happens to be aligned there too, loads of the unit's own size otherwise -- and unit by unit at its two edges.
// No atomics; an idle slot reads no input and writes only its count.
//   gate_reset_kernel   the header (magic, B, the uvad_cuts_cfg, unit size, ring length) and every slot idle; the rings are not touched:
//                       a session reads only what it has written
//   gate_step_kernel    the step above
#include <climits>
#include <cstddef>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

static_assert(sizeof(GateHeader) == 256 && sizeof(GateSlot) == 64 && sizeof(GateSeg) == 32 && sizeof(uvad_gate_seg) == 32, "uvad_gate state and record");
static_assert(offsetof(uvad_gate_seg, offset) == offsetof(GateSeg, offset) && offsetof(uvad_gate_seg, n_stored) == offsetof(GateSeg, n_stored), "uvad_gate_seg");
static_assert(UVAD_GATE_FIRST == 1 && UVAD_GATE_LAST == 2 && UVAD_GATE_LOST == 4 && UVAD_GATE_SHORT == 8, "record flags");

namespace {

__global__ __launch_bounds__(256) void gate_reset_kernel(unsigned *state, int B, CutsCfgInt q, int unit_bytes, int history) {
    const long long n = (long long)((sizeof(GateHeader) + (size_t)B * sizeof(GateSlot)) / sizeof(unsigned));
    const unsigned long long rb = gate_ring_bytes(unit_bytes, history);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        unsigned v = 0u;
        if (i == 0) v = GATE_MAGIC;
        else if (i == 1) v = (unsigned)B;
        else if (i == 2) v = (unsigned)q.pad;
        else if (i == 3) v = (unsigned)q.max_len;
        else if (i == 4) v = (unsigned)q.min_len;
        else if (i == 5) v = (unsigned)q.hop;
        else if (i == 6) v = (unsigned)q.lead;
        else if (i == 7) v = (unsigned)q.tail;
        else if (i == 8) v = (unsigned)unit_bytes;
        else if (i == 9) v = (unsigned)history;
        else if (i == 10) v = (unsigned)(rb & 0xffffffffull);
        else if (i == 11) v = (unsigned)(rb >> 32);
        state[i] = v;
    }
}

// n units from src (nullptr: zeros) to dst, by all lanes of the workgroup; dst and src are unit-aligned, nothing more is assumed
template <class G> __device__ __forceinline__ void gate_copy_span(G *dst, const G *src, long long n, int tid) {
    constexpr int V = 16 / (int)sizeof(G);
    if (n <= 0) return;
    long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(G));
    head = head < n ? head : n;
    const long long body = (n - head) / V, tail0 = head + body * V;
    for (long long i = tid; i < head; i += GATE_THREADS) dst[i] = src ? src[i] : (G)0;
    G *d = dst + head;
    const G *s = src ? src + head : nullptr;
    const bool same = s && (reinterpret_cast<uintptr_t>(s) & 15u) == 0;
    for (long long v = tid; v < body; v += GATE_THREADS) {
        union { G e[V]; uint4 q; } u;
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
    for (long long i = tail0 + tid; i < n; i += GATE_THREADS) dst[i] = src ? src[i] : (G)0;
}

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

    // 2 the walk: lane 0's variables below are the slot
    long long sent = st.sent, pf = st.pf, c = st.c, F = st.F, out_off = 0;
    int idx = st.idx, mode = st.mode, started = st.started, nrec = 0;
    // the current piece, k frames so far, delivers its samples up to the absolute position upto
    auto record = [&](int flags, long long k, long long upto) {
        long long first = pf * hop - lead;
        first = first < 0 ? 0 : first;
        long long total = upto - first;
        total = total < 0 ? 0 : total;
        long long n = total - sent;
        n = n < 0 ? 0 : n;
        if (!(flags & UVAD_GATE_LAST) && n == 0) return;                    // an open piece with nothing new says nothing
        const long long src = first + sent;
        if (!started) flags |= UVAD_GATE_FIRST;
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
    };
    auto cover = [&](long long g) {                                         // frames below g are known to lie inside the interval
        while (W && g - pf >= W) close(W);
    };
    auto known = [&]() { return mode == EP_SPEECH ? F : (c + P < F ? c + P : F); };

    __syncthreads();                                                        // the chunk is in the ring, the first labels in LDS
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
    if (tid == 0) {
        if (mode != EP_IDLE) {
            const long long g = known();
            if (ending) {
                cover(g);
                if (g > pf) close(g - pf);
            } else if (g > pf) {
                const long long upto = g * hop < A ? g * hop : A;
                record(0, g - pf, upto);
            }
        }
        GateSlot o{};
        o.wp = wp;
        if (!ending) {
            o.A = A; o.sent = sent; o.F = (int)F; o.c = (int)c; o.pf = (int)pf; o.idx = idx; o.mode = mode; o.started = started; o.live = 1;
        }
        *S = o;
        a.seg_counts[b] = nrec;
        sh_nrec = nrec < a.max_seg ? nrec : a.max_seg;
    }
    __syncthreads();                                                        // lane 0's records are visible to the workgroup

    // 3 the copy
    if (!seg) return;
    const int lim = sh_nrec;
    G *orow = reinterpret_cast<G *>(a.out) + (size_t)b * (size_t)a.ld_out;
    long long off = 0;
    for (int r = 0; r < lim; ++r) {
        const GateSeg q = seg[r];
        const long long ns = q.n_stored;
        if (ns <= 0) continue;
        long long first = (long long)q.first_frame * hop - lead;
        first = first < 0 ? 0 : first;
        const long long p0 = first + q.offset;                              // the fragment is samples [p0, p0 + ns) of the session, p0 + ns <= A
        long long gone = A - H - p0;                                        // samples that have left the ring: zeros
        gone = gone < 0 ? 0 : gone > ns ? ns : gone;
        G *dst = orow + off;
        gate_copy_span<G>(dst, nullptr, gone, tid);
        const long long m = ns - gone, back = A - (p0 + gone);              // sample p sits A - p places behind the write position
        if (m > 0 && back >= m && back <= H) {
            long long at = wp - back;
            at = at < 0 ? at + H : at;
            const long long m1 = m < H - at ? m : H - at;
            gate_copy_span(dst + gone, ring + at, m1, tid);
            gate_copy_span(dst + gone + m1, ring, m - m1, tid);
        }
        off += ns;
    }
}

}  // namespace

hipError_t launch_gate_reset(void *state, int B, const CutsCfgInt &q, int unit_bytes, int history, hipStream_t s) {
    if (!state || B <= 0 || (unit_bytes != 2 && unit_bytes != 4) || history < 1) return hipErrorInvalidValue;
    const long long n = (long long)((sizeof(GateHeader) + (size_t)B * sizeof(GateSlot)) / sizeof(unsigned));
    const long long g = (n + 255) / 256;
    hipLaunchKernelGGL(gate_reset_kernel, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(256), 0, s, reinterpret_cast<unsigned *>(state), B, q, unit_bytes,
                       history);
    return hipGetLastError();
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
