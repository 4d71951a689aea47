// energy_order.h -- the one energy reduction of the augmentation stages: E(x, n) = (sum (double)x (double)x) / n in the order include/uvad.h
// fixes for uvad_mix_* and uvad_reverb_* borrows (mix.hip, reverb.hip), and the guarded row loads both stages read a batch with.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/uvad.h"
#include "uvad_internal.h"

namespace uvad {

__device__ __forceinline__ long long mix_row_len(const long long *nsamp, long long b, long long S) {
    if (!nsamp) return S;
    const long long n = nsamp[b];
    return n < 0 ? 0 : n > S ? S : n;
}

// samples i .. i + 3 of a row with n valid samples, as f32; an element at or past n is +0 and is not read.  vec: the row starts on a
// 16-byte (f32) / 8-byte (int16) boundary, and i is a multiple of 4
template <int FMT>
__device__ __forceinline__ float4 mix_load4(const void *row, long long i, long long n, bool vec) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (FMT == UVAD_INGEST_F32) {
        const float *p = reinterpret_cast<const float *>(row) + i;
        if (vec && i + 4 <= n) return *reinterpret_cast<const float4 *>(p);
        if (i < n) v.x = p[0];
        if (i + 1 < n) v.y = p[1];
        if (i + 2 < n) v.z = p[2];
        if (i + 3 < n) v.w = p[3];
    } else {
        constexpr float k = 1.0f / 32768.0f;
        const short *p = reinterpret_cast<const short *>(row) + i;
        if (vec && i + 4 <= n) {
            const short4 q = *reinterpret_cast<const short4 *>(p);
            return make_float4((float)q.x * k, (float)q.y * k, (float)q.z * k, (float)q.w * k);
        }
        if (i < n) v.x = (float)p[0] * k;
        if (i + 1 < n) v.y = (float)p[1] * k;
        if (i + 2 < n) v.z = (float)p[2] * k;
        if (i + 3 < n) v.w = (float)p[3] * k;
    }
    return v;
}

template <int FMT>
__device__ __forceinline__ bool mix_row_vec(const void *row) {
    return (reinterpret_cast<uintptr_t>(row) & (FMT == UVAD_INGEST_F32 ? 15 : 7)) == 0;
}

// The sum of squares of a row's n samples by one workgroup of MIX_LANES threads, every thread calling: lane t = (i / 4) mod 1024 adds its
// samples in increasing i, the lanes are folded by a tree.  The sum is thread 0's return value; the others' is not a sum.  s_lo / s_hi:
// MIX_LANES / 64 words of LDS each, free again after the next barrier.
template <int FMT>
__device__ __forceinline__ double mix_energy_sum(const void *row, long long n, int *s_lo, int *s_hi) {
    const int t = threadIdx.x;
    const bool vec = mix_row_vec<FMT>(row);
    double acc = 0.0;
    for (long long c0 = 0; c0 < n; c0 += 4LL * MIX_CHUNK) {     // four passes of the lanes in flight; the additions stay in index order
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = mix_load4<FMT>(row, c0 + (long long)u * MIX_CHUNK + 4 * t, n, vec);
#pragma unroll
        for (int u = 0; u < 4; ++u) {                           // a group past n is four +0: adding them changes no bit of a sum >= +0
            acc += (double)v[u].x * (double)v[u].x;
            acc += (double)v[u].y * (double)v[u].y;
            acc += (double)v[u].z * (double)v[u].z;
            acc += (double)v[u].w * (double)v[u].w;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);   // lanes t .. t + 63 of one wave: t += t + o
    if ((t & 63) == 0) { s_lo[t >> 6] = __double2loint(acc); s_hi[t >> 6] = __double2hiint(acc); }
    __syncthreads();
    double w = 0.0;
    if (t < 64) {
        w = t < MIX_LANES / 64 ? __hiloint2double(s_hi[t], s_lo[t]) : 0.0;
#pragma unroll
        for (int o = MIX_LANES / 128; o > 0; o >>= 1) w += __shfl_down(w, o);   // the 16 wave sums: j += j + o
    }
    return w;
}

}  // namespace uvad
