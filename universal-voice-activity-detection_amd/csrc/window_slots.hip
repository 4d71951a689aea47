// window_slots.hip -- the slot pools of both window families (uvad_window_slots_*, uvad_window_wav_slots_*, include/uvad.h).
//
// A pool of B slots advances in lockstep like a window stream group, but every slot holds its own session: a per-step flag byte starts
// and ends sessions, and every per-slot quantity -- samples and frames since the session's start, whether the slot is live, the PCM
// tail's ping-pong parity -- lives on the DEVICE (SlotCounters).  The host passes the same launch arguments to every step, so a graph
// captured around any step replays for all later ones, warm-ups and session changes included.
//
// Each step's first kernel (slot_stage_kernel for log-mel, wav_slot_assemble_kernel for the waveform model) applies the flags to the
// counters it reads and writes the slot's SlotPlan into the workspace; every later kernel of the step reads that plan, and the last one
// (slot_emit_kernel) commits the counters.  No kernel reads a counter another kernel of the same step writes.
//
//   slot_stage_kernel        log-mel: an ALIGNED staging row per slot, its frames side by side -- frame j of row b is samples
//                            [j frame_len, (j + 1) frame_len), the slot's new frame j taken from the stream's virtual [tail | chunk]
//                            row (fbank.hip, FbankArgs::vs_*; the first chunk of a session reflected on the left) -- so that the
//                            unchanged feature kernel, run on plain rows with snip_edges = 1 and frame_shift = frame_len, computes the
//                            slot's new frames at columns 0 .. k_b - 1 with the bits of the stream's own step (frames go through the
//                            transform in pairs: an odd k_b's last frame gets a copy of itself as its partner, as a stream's lone last
//                            frame does); and the next tail, tails[par ^ 1] from tails[par], par = step & 1.
//   slot_assemble_kernel     log-mel: commits the k_b new frames to the slot's ring and writes its window of Tw_b = min(e_b, W) frames
//                            left-aligned into the first projection's operand (window_assemble_kernel's layouts), zero past Tw_b;
//                            lens[b] = Tw_b.  With plan == nullptr: the read-only features tap.
//   wav_slot_assemble_kernel waveform: commits the chunk to the slot's PCM ring and writes its window of Sw_b = R + J (Tw_b - 1) samples
//                            left-aligned into [B][Sw_max], zero past Sw_b; nsamp[b] = Sw_b (0 for an idle slot or no frame yet).
//   slot_emit_kernel         both: copies the rows [r0_b, r0_b + n_b) of the classifier's [B][W] outputs to columns 0 .. n_b - 1,
//                            writes counts[b] = n_b and commits the counters.
// Idle slots read nothing of their chunk row.  Global memory only: no LDS, no FLAT, no scratch (tests/test_abi_window_slots.py).
#include "uvad_internal.h"

namespace uvad {

namespace {

int slot_grid(long long n, long long cap) {
    const long long g = (n + 255) / 256;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

// The flags applied to a slot's counters: whether the slot holds a session this step, and the session's samples / frames before it.
struct SlotStart { int live, first, end; long long n_prev, e_prev; };
__device__ inline SlotStart slot_start(const uint8_t *flags, const SlotCounters &ctr, int b) {
    const int f = flags ? flags[b] : 0;
    SlotStart s;
    s.end = (f & 2) ? 1 : 0;
    if (f & 1) {   // START: whatever the slot held is dropped
        s.live = 1; s.first = 1; s.n_prev = 0; s.e_prev = 0;
    } else if (ctr.active[b]) {
        s.live = 1; s.n_prev = ctr.n[b]; s.e_prev = ctr.e[b]; s.first = s.n_prev == 0;
    } else {
        s.live = 0; s.first = 0; s.end = 0; s.n_prev = 0; s.e_prev = 0;
    }
    return s;
}

// Emission of a live slot with e_prev -> e frames: [max(0, e_prev - L), max(0, e - L)), or [max(0, e_prev - L), e) on its END step; the
// rows of the window [e - Tw, e) that hold them.  L + kmax <= W (checked at reset) keeps r0 >= 0 and n_emit <= L + kmax.
__device__ inline void slot_emission(SlotPlan &p, int W, int L) {
    p.Tw = (int)(p.e < W ? p.e : W);
    const long long f0 = p.e_prev - L > 0 ? p.e_prev - L : 0;
    const long long f1 = p.end ? p.e : (p.e - L > 0 ? p.e - L : 0);
    p.n_emit = (int)(f1 - f0);
    p.r0 = (int)(f0 - (p.e - p.Tw));
}

// ---- log-mel --------------------------------------------------------------------------------------------------------------------

__device__ inline SlotPlan logmel_plan(const SlotStageArgs &a, int b) {
    const SlotStart s = slot_start(a.flags, a.ctr, b);
    SlotPlan p{};
    if (!s.live) return p;
    p.live = 1; p.first = s.first; p.end = s.end; p.e_prev = s.e_prev;
    const int L = a.frame_len, sh = a.shift;
    p.n = s.n_prev + a.chunk_len;
    // frame t spans [t sh - n_left, t sh - n_left + L): complete once n >= t sh - n_left + L (stream_plan in uvad_api.hip)
    const long long f_hi = p.n + a.n_left - L >= 0 ? (p.n + a.n_left - L) / sh : -1;
    long long k = f_hi - (s.e_prev - 1);
    if (k < 0) k = 0;
    p.k = (int)k;
    p.e = s.e_prev + k;
    // where the first new frame starts in the virtual row [tail (L samples) | chunk]: in (0, max(sh, L - n_left)]
    p.offset = k > 0 ? (int)(s.e_prev * sh - a.n_left - (s.n_prev - L)) : 0;
    slot_emission(p, a.W, a.L);
    return p;
}

__global__ __launch_bounds__(256) void slot_stage_kernel(SlotStageArgs a) {
    const int b = blockIdx.y;
    const SlotPlan p = logmel_plan(a, b);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.plan[b] = p;
    const int L = a.frame_len;
    const int par = (int)(a.ctr.step[0] & 1);
    const float *chunk = a.chunk + (size_t)b * a.chunk_len;
    const float *tail_in = a.tails + ((size_t)par * a.B + b) * L;
    float *tail_out = a.tails + ((size_t)(par ^ 1) * a.B + b) * L;
    float *row = a.staging + (size_t)b * a.row;
    // sample q of the virtual row [tail | chunk] (fbank.hip vs_abs): the first chunk of a session mirrors its head, edge sample included
    auto virt = [&](int q) -> float {
        if (q >= L) return q - L < a.chunk_len ? chunk[q - L] : 0.0f;
        if (p.first) {
            const int m = L - q;
            return (m <= a.n_left && m - 1 < a.chunk_len) ? chunk[m - 1] : 0.0f;
        }
        return tail_in[q];
    };
    const int items = a.row + (p.live ? L : 0);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += gridDim.x * blockDim.x) {
        if (i < a.row) {
            // frame j of the row is samples [j L, (j + 1) L): the slot's new frame j for j < k, for odd k a copy of frame k - 1 at j = k
            // (the feature kernel transforms frames in pairs (2i, 2i + 1), and a stream's lone last frame is paired with itself), zero
            // past them; an idle slot's row is all zeros (its chunk row is never read)
            const int j = i / L, q = i - j * L;
            const int src = j < p.k ? j : (j == p.k && (p.k & 1)) ? j - 1 : -1;
            row[i] = p.live && src >= 0 ? virt(p.offset + src * a.shift + q) : 0.0f;
        } else {
            const int q = i - a.row;
            tail_out[q] = virt(a.chunk_len + q);
        }
    }
}

__global__ __launch_bounds__(256) void slot_assemble_kernel(SlotAssembleArgs a) {
    const int W = a.W;
    const int q4 = (a.planes ? a.Fp : a.F) / 4;
    const long long rows = a.planes ? (long long)a.tiles * W * SEQ_TILE : (long long)a.B * W;
    const long long n = rows * q4;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < a.B) a.lens[gid] = a.plan ? a.plan[gid].Tw : a.ctr.tw_last[gid];
    for (long long i = gid; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / q4;
        const int c = (int)(i - m * q4) * 4;
        int b, t;   // slot, window row
        if (a.planes) {
            const long long per_tile = (long long)W * SEQ_TILE;
            const int tile = (int)(m / per_tile);
            const int rem = (int)(m - (long long)tile * per_tile);
            t = rem / SEQ_TILE;
            b = tile * SEQ_TILE + (rem - t * SEQ_TILE);
        } else {
            b = (int)(m / W);
            t = (int)(m - (long long)b * W);
        }
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < a.B && c < a.F) {
            long long e, e_new;
            int Tw, k;
            if (a.plan) {
                const SlotPlan &p = a.plan[b];
                e = p.e; e_new = p.e_prev; Tw = p.Tw; k = p.k;
            } else {   // the tap: the window the last step classified, nothing new
                e = a.ctr.e[b]; e_new = e; Tw = a.ctr.tw_last[b]; k = 0;
            }
            if (t < Tw) {
                const long long f = e - Tw + t;   // frame of the session
                float *slot = a.ring + ((size_t)b * W + (size_t)(f % W)) * a.F + c;
                if (f >= e_new && k > 0) {
                    v = *reinterpret_cast<const float4 *>(a.newf + ((size_t)b * a.kmax + (size_t)(f - e_new)) * a.F + c);
                    *reinterpret_cast<float4 *>(slot) = v;
                } else {
                    v = *reinterpret_cast<const float4 *>(slot);
                }
            }
        }
        if (!a.planes) {
            *reinterpret_cast<float4 *>(a.out + ((size_t)b * W + t) * a.F + c) = v;
            continue;
        }
        // the split of split_features_kernel: a ~= hi + lo * 2^-11
        const float e4[4] = {v.x, v.y, v.z, v.w};
        unsigned short h[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const _Float16 hh = (_Float16)e4[j];
            const _Float16 ll = (_Float16)((e4[j] - (float)hh) * 2048.0f);
            h[j] = __builtin_bit_cast(unsigned short, hh);
            l[j] = __builtin_bit_cast(unsigned short, ll);
        }
        const size_t o = plane_index(m, c, a.Fp);
        *reinterpret_cast<uint2 *>(a.xh + o) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
        *reinterpret_cast<uint2 *>(a.xl + o) = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
    }
}

// ---- waveform -------------------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(256) void wav_slot_assemble_kernel(WavSlotArgs a) {
    const int b = blockIdx.y;
    const SlotStart s = slot_start(a.flags, a.ctr, b);
    SlotPlan p{};
    long long lo = 0;
    if (s.live) {
        p.live = 1; p.first = s.first; p.end = s.end; p.e_prev = s.e_prev;
        p.n = s.n_prev + a.chunk_len;
        p.e = p.n < a.R ? 0 : (p.n - a.R) / a.J + 1;
        p.k = (int)(p.e - s.e_prev);
        slot_emission(p, a.W, a.L);
        lo = (long long)a.J * (p.e - p.Tw);
    }
    const long long Sw = p.Tw > 0 ? (long long)a.R + (long long)a.J * (p.Tw - 1) : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.plan[b] = p;
        a.nsamp[b] = Sw;
    }
    const long long n_prev = s.n_prev;
    const long long cbase = n_prev % a.ring_len, wbase = lo % a.ring_len;
    const T *chunk = static_cast<const T *>(a.chunk) + (size_t)b * a.chunk_len;
    T *ring = static_cast<T *>(a.ring) + (size_t)b * a.ring_len;
    T *out = static_cast<T *>(a.out) + (size_t)b * a.Sw_max;
    const int commit = s.live ? a.chunk_len : 0;   // an idle slot's chunk row is never read
    const int items = commit + a.Sw_max;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += gridDim.x * blockDim.x) {
        if (i < commit) {
            long long slot = cbase + i;
            if (slot >= a.ring_len) slot -= a.ring_len;
            ring[slot] = chunk[i];
            continue;
        }
        const int j = i - commit;
        T v = T(0);
        if (j < Sw) {
            const long long q = lo + j;   // sample of the session, < n
            if (q >= n_prev) {
                if (q - n_prev < a.chunk_len) v = chunk[q - n_prev];
            } else {
                long long slot = wbase + j;
                if (slot >= a.ring_len) slot -= a.ring_len;
                v = ring[slot];
            }
        }
        out[j] = v;
    }
}

// ---- both -----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void slot_emit_kernel(SlotEmitArgs a) {
    const int b = blockIdx.x;
    const SlotPlan p = a.plan[b];
    for (int j = threadIdx.x; j < p.n_emit; j += blockDim.x) {
        const size_t src = (size_t)b * a.W + p.r0 + j, dst = (size_t)b * a.ld_out + j;
        if (a.logits) a.logits[dst] = a.logits_in[src];
        if (a.probs) a.probs[dst] = a.probs_in[src];
    }
    if (threadIdx.x == 0) {
        a.counts[b] = p.n_emit;
        a.ctr.tw_last[b] = p.Tw;
        if (p.live) {   // an ended slot keeps its counts for the features tap; only START reads them again (as zero)
            a.ctr.n[b] = p.n;
            a.ctr.e[b] = p.e;
            a.ctr.active[b] = p.end ? 0 : 1;
        }
        if (b == 0) a.ctr.step[0] = a.ctr.step[0] + 1;
    }
}

}  // namespace

hipError_t launch_slot_stage(const SlotStageArgs &a, hipStream_t s) {
    if (!a.chunk || !a.tails || !a.staging || !a.plan || !a.ctr.n || !a.ctr.e || !a.ctr.active || !a.ctr.step) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.chunk_len < a.n_left || a.frame_len <= 0 || a.shift <= 0 || a.row < 2 * a.frame_len || a.row % (2 * a.frame_len)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_stage_kernel, dim3(slot_grid(a.row + a.frame_len, 4 + 4096 / a.B), a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_slot_assemble(const SlotAssembleArgs &a, hipStream_t s) {
    if (a.B <= 0 || a.W <= 0 || a.F <= 0 || a.F % 4 || !a.ring || !a.lens || !a.ctr.e || !a.ctr.tw_last) return hipErrorInvalidValue;
    if (a.plan && (!a.newf || a.kmax <= 0)) return hipErrorInvalidValue;
    if (a.planes ? (!a.xh || !a.xl || a.Fp < a.F || a.Fp % 16 || a.tiles * SEQ_TILE < a.B) : !a.out) return hipErrorInvalidValue;
    const long long rows = a.planes ? (long long)a.tiles * a.W * SEQ_TILE : (long long)a.B * a.W;
    const long long n = rows * ((a.planes ? a.Fp : a.F) / 4);
    hipLaunchKernelGGL(slot_assemble_kernel, dim3(slot_grid(n > a.B ? n : a.B, 4096)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wav_slot_assemble(const WavSlotArgs &a, int is_i16, hipStream_t s) {
    if (!a.chunk || !a.ring || !a.out || !a.nsamp || !a.plan || !a.ctr.n || !a.ctr.e || !a.ctr.active) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.chunk_len <= 0 || a.J <= 0 || a.R <= 0 || a.W <= 0 || a.Sw_max != a.R + a.J * (a.W - 1))
        return hipErrorInvalidValue;
    // every ring slot one launch touches is distinct: the chunk plus the window's reach back from n (< Sw + J samples)
    if (a.ring_len < a.chunk_len || a.ring_len < (long long)a.Sw_max + a.J) return hipErrorInvalidValue;
    const long long items = (long long)a.chunk_len + a.Sw_max;
    if (items > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)slot_grid(items, 4 + 4096 / a.B), (unsigned)a.B);
    if (is_i16) hipLaunchKernelGGL(wav_slot_assemble_kernel<int16_t>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(wav_slot_assemble_kernel<float>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_slot_emit(const SlotEmitArgs &a, hipStream_t s) {
    if (a.B <= 0 || a.W <= 0 || !a.plan || !a.counts || !a.ctr.n || !a.ctr.e || !a.ctr.active || !a.ctr.tw_last || !a.ctr.step)
        return hipErrorInvalidValue;
    if ((a.logits && !a.logits_in) || (a.probs && !a.probs_in) || (!a.logits && !a.probs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_emit_kernel, dim3(a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
