// fuse.hip -- channel fusion on the device (uvad_fuse_*, include/uvad.h): the rows the ingest stage made of one recording's channels put
// back together.  Group g of the configuration is member slots [first[g], first[g + 1]); slot j reads input row members[j].  Per group and
// frame: the fused value (MAX, weighted MEAN, weighted VOTE), its label, the position of the member that heard it best, and four counters
// per member slot.  Everything is bit-defined (the MEAN / VOTE sums run in f64 in slot order); no atomics: the same calls give the same bytes.
//   fuse_kernel       (an instance per mode) one workgroup per (group, tile of 1024 frames), strided past the grid cap; lanes along time,
//                     four consecutive frames a lane, members in an inner loop.  A member's four frames come by one 16-byte load when the row's base is
//                     16-byte aligned and all four lie below the row's length, and one by one otherwise: the arithmetic per frame is the
//                     same, so the output does not depend on which path ran.  Columns at or past a row's length are never read, rows of
//                     length 0 never touched, output columns at or past the group's length never written.  With d_stats a second pass over
//                     the members (their tile is in L2) turns each counter's predicate into ballots and population counts: one
//                     FusePartial per (member slot, tile, wave) in the workspace.
//   fuse_fold_kernel  one wave per member slot: lanes stride over the slot's partials, a shuffle tree sums them, lane 0 ADDS into d_stats.
//   fuse_pick_kernel  one wave per cut of a table made from the fused labels: d_best goes by 64 frames at a time, one ballot per member
//                     position present in the 64, lane k holds the count of positions k, k + 64, ...; a shuffle tree takes the largest
//                     count, ties to the lowest position.
// Bytes per fused frame of M members: 4 M read; 4 (fused) + 1 (label) + 1 (best) written.
#include <cstddef>
#include <cstdint>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

static_assert(UVAD_FUSE_MAX == 0 && UVAD_FUSE_MEAN == 1 && UVAD_FUSE_VOTE == 2 && FUSE_STATS_WORDS == UVAD_FUSE_STATS_WORDS &&
              FUSE_MAX_MEMBERS == UVAD_FUSE_MAX_MEMBERS && sizeof(FusePartial) == 16, "include/uvad.h");

namespace {

typedef unsigned long long u64;

// p ranks strictly above cur: NaN above everything, and nothing above a NaN (so ties, NaN against NaN included, keep the lower position)
__device__ __forceinline__ bool fuse_above(float p, float cur) { return !(cur != cur) && (p != p || p > cur); }

__device__ __forceinline__ bool fuse_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the four frames t .. t + 3 of a member row of n frames, n > t; frames at or past n are not read (and come back 0)
__device__ __forceinline__ void fuse_load4(const float *src, int left, float p[4]) {
    if (left >= 4 && fuse_aligned16(src)) {
        const float4 v = *reinterpret_cast<const float4 *>(src);
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = k < left ? src[k] : 0.0f;
    }
}

template <int MODE> __global__ __launch_bounds__(FUSE_THREADS) void fuse_kernel(FuseArgs a) {
    __shared__ int s_row[FUSE_THREADS], s_n[FUSE_THREADS];
    __shared__ float s_w[FUSE_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.tiles * FUSE_WAVES;
    const long long items = (long long)a.G * a.tiles;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int g = (int)(it / a.tiles), tile = (int)(it % a.tiles);
        const int j0 = a.first[g], M = a.first[g + 1] - j0;     // 1 .. 255, checked at configure
        __syncthreads();                                         // the item before this one is done with the three arrays
        if (tid < M) {
            const int row = a.members[j0 + tid];
            int n = a.T;
            if (a.lens) { n = a.lens[row]; n = n < 0 ? 0 : n > a.T ? a.T : n; }
            s_row[tid] = row; s_n[tid] = n; s_w[tid] = a.weights ? a.weights[j0 + tid] : 1.0f;
        }
        __syncthreads();
        int L = 0;
        for (int j = 0; j < M; ++j) L = s_n[j] > L ? s_n[j] : L;
        if (tile == 0 && tid == 0) {
            a.glens[g] = L;
            if (a.flags_out) {
                unsigned f = 0;
                for (int j = 0; j < M; ++j) f |= a.flags_in[s_row[j]];
                a.flags_out[g] = (uint8_t)f;
            }
        }
        const int t0 = tile * FUSE_TILE;                         // T <= 2^30: t0 + 1023 fits
        if (t0 >= L) {                                           // nothing of this tile exists: its partials are zeros, nothing else is touched
            if (a.stats)
                for (int i = tid; i < M * FUSE_WAVES; i += FUSE_THREADS)
                    a.part[(size_t)(j0 + i / FUSE_WAVES) * P + tile * FUSE_WAVES + i % FUSE_WAVES] = FusePartial{0u, 0u, 0u, 0u};
            continue;
        }
        const int t = t0 + tid * 4;
        const int nf = L - t < 0 ? 0 : L - t > 4 ? 4 : L - t;    // my frames below the group's length
        float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int bi[4] = {-1, -1, -1, -1};
        bool lab[4] = {false, false, false, false};
        if (nf > 0) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0}, W[4] = {0.0, 0.0, 0.0, 0.0};
            for (int j = 0; j < M; ++j) {
                const int left = s_n[j] - t;
                if (left <= 0) continue;                         // no frame of mine is valid in this member (a row of length 0 is never touched)
                float p[4];
                fuse_load4(a.in + (size_t)s_row[j] * a.ld_in + t, left, p);
                const double w = (double)s_w[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) {                    // selects, not branches: one straight line per frame
                    const bool valid = k < left;
                    const bool take = valid && (bi[k] < 0 || fuse_above(p[k], bv[k]));
                    bv[k] = take ? p[k] : bv[k];
                    bi[k] = take ? j : bi[k];
                    if (MODE != UVAD_FUSE_MAX) {
                        const double x = MODE == UVAD_FUSE_MEAN ? (double)p[k] : !(p[k] < a.q.threshold) ? 1.0 : 0.0;
                        acc[k] = valid ? acc[k] + w * x : acc[k];
                        W[k] = valid ? W[k] + w : W[k];
                    }
                }
            }
            float f[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (MODE == UVAD_FUSE_MAX) {
                    f[k] = bv[k];                                // the best member's value as it is, a NaN's payload included
                } else {
                    f[k] = W[k] == 0.0 ? 0.0f : (float)(acc[k] / W[k]);
                    if (f[k] != f[k]) f[k] = __uint_as_float(0x7fc00000u);   // one NaN, whatever sign the sum gave it
                }
                lab[k] = !(f[k] < a.q.decide);
            }
            float *fo = a.fused + (size_t)g * a.ld_f + t;
            if (nf == 4 && fuse_aligned16(fo)) {
                *reinterpret_cast<float4 *>(fo) = make_float4(f[0], f[1], f[2], f[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (k < nf) fo[k] = f[k];
            }
            if (a.labels) {
                uint8_t *lo = a.labels + (size_t)g * a.ld_l + t;
                if (nf == 4 && (reinterpret_cast<uintptr_t>(lo) & 3) == 0) {
                    *reinterpret_cast<uchar4 *>(lo) = make_uchar4(lab[0], lab[1], lab[2], lab[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (k < nf) lo[k] = lab[k] ? 1 : 0;
                }
            }
            if (a.best) {
                uint8_t *bo = a.best + (size_t)g * a.ld_b + t;
                if (nf == 4 && (reinterpret_cast<uintptr_t>(bo) & 3) == 0) {
                    *reinterpret_cast<uchar4 *>(bo) = make_uchar4((uint8_t)bi[0], (uint8_t)bi[1], (uint8_t)bi[2], (uint8_t)bi[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (k < nf) bo[k] = (uint8_t)bi[k];
                }
            }
        }
        if (!a.stats) continue;
        // the counters: every lane of the workgroup walks the members (the ballots want whole waves)
        for (int j = 0; j < M; ++j) {
            const int left = s_n[j] - t;
            float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (left > 0) fuse_load4(a.in + (size_t)s_row[j] * a.ld_in + t, left, p);
            unsigned c_valid = 0, c_speech = 0, c_agree = 0, c_best = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool valid = k < left, own = valid && !(p[k] < a.q.threshold);
                c_valid += __popcll((u64)__ballot(valid));
                c_speech += __popcll((u64)__ballot(own));
                c_agree += __popcll((u64)__ballot(valid && own == lab[k]));
                c_best += __popcll((u64)__ballot(valid && bi[k] == j));
            }
            if (lane == 0) a.part[(size_t)(j0 + j) * P + tile * FUSE_WAVES + wave] = FusePartial{c_valid, c_speech, c_agree, c_best};
        }
    }
}

__device__ __forceinline__ u64 fuse_wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                                    // lane 0 holds the sum
}

__global__ __launch_bounds__(256) void fuse_fold_kernel(FuseArgs a) {
    const int lane = threadIdx.x & 63;
    const int P = a.tiles * FUSE_WAVES;
    for (long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); j < a.N; j += (long long)gridDim.x * 4) {
        u64 s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (int i = lane; i < P; i += 64) {
            const FusePartial q = a.part[(size_t)j * P + i];
            s0 += q.valid; s1 += q.speech; s2 += q.agree; s3 += q.best;
        }
        s0 = fuse_wave_sum(s0); s1 = fuse_wave_sum(s1); s2 = fuse_wave_sum(s2); s3 = fuse_wave_sum(s3);
        if (lane == 0) {
            u64 *w = a.stats + (size_t)j * FUSE_STATS_WORDS;
            w[0] += s0; w[1] += s1; w[2] += s2; w[3] += s3;
        }
    }
}

__global__ __launch_bounds__(256) void fuse_pick_kernel(FusePickArgs a) {
    const int lane = threadIdx.x & 63;
    int m = *a.total;
    m = m < 0 ? 0 : m < a.max_cuts ? m : a.max_cuts;
    for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += (long long)gridDim.x * 4) {
        CutRecord q = a.table[i];
        const int g = q.row;
        if (g < 0 || g >= a.G) {                                 // not a row of the fused labels: copied as it is
            if (lane == 0) {
                if (a.out_table) a.out_table[i] = q;
                if (a.pick) a.pick[i] = -1;
            }
            continue;
        }
        const int j0 = a.first[g], M = a.first[g + 1] - j0;
        const long long lo = q.first_frame < 0 ? 0 : q.first_frame;
        long long hi = (long long)q.first_frame + q.n_frames;
        hi = hi > a.ld_b ? a.ld_b : hi;                          // a table from the fused labels never asks for more
        const uint8_t *row = a.best + (size_t)g * a.ld_b;
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;                       // lane k: the frames won by positions k, k + 64, k + 128, k + 192
        for (long long f0 = lo; f0 < hi; f0 += 64) {
            const long long f = f0 + lane;
            const bool in = f < hi;
            const int b = in ? (int)row[f] : -1;
            u64 rem = (u64)__ballot(in);
            while (rem) {                                        // one ballot per position present among the 64
                const int v = __shfl(b, __ffsll((long long)rem) - 1);
                const u64 hit = (u64)__ballot(b == v);
                const int c = __popcll(hit);
                if (lane == (v & 63)) {
                    const int w = v >> 6;
                    c0 += w == 0 ? c : 0; c1 += w == 1 ? c : 0; c2 += w == 2 ? c : 0; c3 += w == 3 ? c : 0;
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
        if (lane == 0) {                                         // M >= 1: position 0 always stands, so bp is a position of the group
            if (a.pick) a.pick[i] = bp;
            if (a.out_table) {
                q.row = a.members[j0 + bp];
                a.out_table[i] = q;
            }
        }
    }
}

}  // namespace

hipError_t launch_fuse(const FuseArgs &a, hipStream_t s) {
    if (!a.first || !a.members || !a.in || !a.fused || !a.glens || !a.part || a.G < 1 || a.N < 1 || a.T < 1 || a.T > FUSE_MAX_T ||
        a.tiles != fuse_tiles(a.T) || a.ld_in < a.T || a.ld_f < a.T || (a.labels && a.ld_l < a.T) || (a.best && a.ld_b < a.T) ||
        (a.flags_in == nullptr) != (a.flags_out == nullptr))
        return hipErrorInvalidValue;
    long long blocks = (long long)a.G * a.tiles;
    blocks = blocks > FUSE_MAX_BLOCKS ? FUSE_MAX_BLOCKS : blocks;
    if (a.q.mode == UVAD_FUSE_MAX) hipLaunchKernelGGL(fuse_kernel<UVAD_FUSE_MAX>, dim3((unsigned)blocks), dim3(FUSE_THREADS), 0, s, a);
    else if (a.q.mode == UVAD_FUSE_MEAN) hipLaunchKernelGGL(fuse_kernel<UVAD_FUSE_MEAN>, dim3((unsigned)blocks), dim3(FUSE_THREADS), 0, s, a);
    else if (a.q.mode == UVAD_FUSE_VOTE) hipLaunchKernelGGL(fuse_kernel<UVAD_FUSE_VOTE>, dim3((unsigned)blocks), dim3(FUSE_THREADS), 0, s, a);
    else return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.stats) return e;
    blocks = ((long long)a.N + 3) / 4;
    blocks = blocks > FUSE_MAX_BLOCKS ? FUSE_MAX_BLOCKS : blocks;
    hipLaunchKernelGGL(fuse_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fuse_pick(const FusePickArgs &a, hipStream_t s) {
    if (!a.first || !a.members || !a.best || !a.total || a.G < 1 || a.ld_b < 1 || a.max_cuts < 0 || (a.max_cuts > 0 && !a.table) ||
        (!a.out_table && !a.pick))
        return hipErrorInvalidValue;
    long long blocks = ((long long)a.max_cuts + 3) / 4;          // one wave per cut, strided past the cap
    blocks = blocks > FUSE_MAX_BLOCKS ? FUSE_MAX_BLOCKS : blocks;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(fuse_pick_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
