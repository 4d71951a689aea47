// sliding.hip -- window assembly and aggregation of sliding-window inference over whole recordings (uvad_sliding_*, include/uvad.h).
//
// A batch of R recordings is covered by N = first[R] windows of at most W frames, hop Hf: global window i with first[r] <= i < first[r + 1]
// is window j = i - first[r] of recording r; it starts at frame j Hf and holds len_j = clamp(T_r - j Hf, 0, W) frames.  first (the
// exclusive prefix of the per-recording window counts) comes from the host, which owns the launch count; T_r is always derived from
// the DEVICE lengths, so a plan that disagrees with them can never make a kernel read outside a recording's row: a window past the
// recording's end is empty, a frame no planned window covers comes out as zero.
//   sliding_assemble_kernel    log-mel: the windows [i0, i0 + Bg) of a classifier launch, cut out of the recordings' continuous
//                              feature rows [R][T][F] and written left-aligned into the first projection's operand exactly as
//                              window_assemble_kernel writes it -- the (hi, lo) f16 planes in split_features_kernel's tile-major layout
//                              and / or canonical f32 rows [Bg][W][F] -- zero past len_j and in the padding sequences; lens[b] = len_j
//   sliding_wav_gather_kernel  waveform: the PCM of the same windows, samples [J Hf j, J Hf j + Sw) clipped to S_r, left-aligned into
//                              [Bg][Sw] (zero past the clipped length); nsamp[b] = that length
//   sliding_aggregate_kernel   out[r][t] = (sum_j w[t - j Hf] p_j[t - j Hf]) / (sum_j w[t - j Hf]) over the windows that cover t, ascending
//                              j, f32 with every product, sum and the quotient rounded once; +0 at t >= T_r and where nothing covers;
//                              frames[r] = T_r
// Global memory only; every thread's reads are bounded by the clamped device lengths.
#include "uvad_internal.h"

namespace uvad {

namespace {

// T_r of recording r from the device lengths: frame counts (int32, clamped to [0, T]) or sample counts of the waveform model (int64,
// clamped to [0, S]; frames(S) = 0 if S < R else (S - R) / J + 1)
__device__ __forceinline__ int sliding_frames(const SlidingPlan &p, int r) {
    if (p.lens) {
        const int v = p.lens[r];
        return v < 0 ? 0 : v > p.T ? p.T : v;
    }
    long long n = p.nsamp[r];
    n = n < 0 ? 0 : n > p.S ? p.S : n;
    const long long f = n < p.R0 ? 0 : (n - p.R0) / p.J + 1;
    return (int)(f > p.T ? p.T : f);
}

// the recording of global window i: first[r] <= i < first[r + 1] (r = R - 1 when i is past the plan's end: its windows are empty)
__device__ __forceinline__ int sliding_seek(const int *first, int R, long long i) {
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// window i -> (r, start frame, len_j); len_j = 0 for anything the device lengths do not back
__device__ __forceinline__ void sliding_window_of(const SlidingPlan &p, long long i, int &r, long long &start, int &len) {
    r = sliding_seek(p.first, p.nrec, i);
    const long long j = i - p.first[r];
    start = j * p.Hf;
    len = 0;
    if (i < p.N && j >= 0 && i < p.first[r + 1]) {
        const long long left = (long long)sliding_frames(p, r) - start;
        len = (int)(left < 0 ? 0 : left > p.W ? p.W : left);
    }
}

__global__ __launch_bounds__(256) void sliding_assemble_kernel(SlidingAssembleArgs a) {
    const SlidingPlan &p = a.plan;
    const int W = p.W;
    const int q4 = (a.planes ? a.Fp : a.F) / 4;
    const long long rows = a.planes ? (long long)a.tiles * W * SEQ_TILE : (long long)a.Bg * W;
    const long long n = rows * q4;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < a.Bg) {
        int r, len;
        long long start;
        sliding_window_of(p, a.i0 + gid, r, start, len);
        a.lens[gid] = len;
    }
    bool bad = false;
    for (long long i = gid; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / q4;
        const int c = (int)(i - m * q4) * 4;
        int b, t;   // window of the group, window row
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
        if (b < a.Bg && c < a.F) {
            int r, len;
            long long start;
            sliding_window_of(p, a.i0 + b, r, start, len);
            if (t < len) v = *reinterpret_cast<const float4 *>(a.feats + ((size_t)r * p.T + (size_t)(start + t)) * a.F + c);   // start + t < T_r <= T
        }
        if (a.out && b < a.Bg && c < a.F) *reinterpret_cast<float4 *>(a.out + ((size_t)b * W + t) * a.F + c) = v;
        if (!a.planes) continue;
        bad |= !(__builtin_fabsf(v.x) < 65504.0f) | !(__builtin_fabsf(v.y) < 65504.0f) | !(__builtin_fabsf(v.z) < 65504.0f) | !(__builtin_fabsf(v.w) < 65504.0f);
        // the split of split_features_kernel: a ~= hi + lo * 2^-11
        const float e4[4] = {v.x, v.y, v.z, v.w};
        unsigned short h[4], l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const _Float16 hh = (_Float16)e4[k];
            const _Float16 ll = (_Float16)((e4[k] - (float)hh) * 2048.0f);
            h[k] = __builtin_bit_cast(unsigned short, hh);
            l[k] = __builtin_bit_cast(unsigned short, ll);
        }
        const size_t o = plane_index(m, c, a.Fp);
        *reinterpret_cast<uint2 *>(a.xh + o) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
        *reinterpret_cast<uint2 *>(a.xl + o) = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
    }
    // caller-supplied features: the device flag of split_features_kernel (a value outside the f16 range sends the first projection to the exact kernel)
    if (a.flag && __builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(a.flag, 1);
}

template <typename T>
__global__ __launch_bounds__(256) void sliding_wav_gather_kernel(SlidingWavArgs a) {
    const SlidingPlan &p = a.plan;
    const int b = blockIdx.y;
    int r, len;
    long long start;
    sliding_window_of(p, a.i0 + b, r, start, len);
    long long Sr = p.nsamp[r];
    Sr = Sr < 0 ? 0 : Sr > p.S ? p.S : Sr;
    const long long s0 = start * p.J;   // len > 0: s0 + R0 <= S_r
    long long ns = 0;
    if (len > 0) {
        ns = Sr - s0;
        if (ns > a.Sw) ns = a.Sw;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.nsamp_out[b] = ns;
    const T *src = static_cast<const T *>(a.pcm) + (size_t)r * p.S + (size_t)(len > 0 ? s0 : 0);
    T *out = static_cast<T *>(a.out) + (size_t)b * a.Sw;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.Sw; i += gridDim.x * blockDim.x) out[i] = i < ns ? src[i] : T(0);
}

__global__ __launch_bounds__(256) void sliding_aggregate_kernel(SlidingAggregateArgs a) {
    const SlidingPlan &p = a.plan;
    const int r = blockIdx.y;
    const int Tr = sliding_frames(p, r);
    const long long f0 = p.first[r];
    long long nw = (long long)p.first[r + 1] - f0;   // planned windows of r, those past N dropped
    if (f0 + nw > p.N) nw = p.N - f0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.frames) a.frames[r] = Tr;
    float *out = a.out + (size_t)r * a.ld_out;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < p.T; t += gridDim.x * blockDim.x) {
        float res = 0.0f;
        if (t < Tr && f0 >= 0) {
            // windows j with j Hf <= t < j Hf + W (t < T_r: len_j reaches t whenever W does), j < nw
            const long long j_lo = t < p.W ? 0 : (t - p.W) / p.Hf + 1;
            long long j_hi = t / p.Hf;
            if (j_hi > nw - 1) j_hi = nw - 1;
            float num = 0.0f, den = 0.0f;
            for (long long j = j_lo; j <= j_hi; ++j) {
                const int k = (int)(t - j * p.Hf);
                const float w = a.weights ? a.weights[k] : 1.0f;
                num = __fadd_rn(num, __fmul_rn(w, a.win[(size_t)(f0 + j) * p.W + k]));
                den = __fadd_rn(den, w);
            }
            if (j_hi >= j_lo) res = __fdiv_rn(num, den);
        }
        out[t] = res;
    }
}

int sliding_grid(long long n, int cap) {
    const long long g = (n + 255) / 256;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

bool plan_ok(const SlidingPlan &p, bool wav) {
    if (!p.first || p.nrec <= 0 || p.nrec > 65535 || p.N < 0 || p.W <= 0 || p.Hf < 1 || p.Hf > p.W || p.T <= 0) return false;
    if (wav) return p.nsamp && !p.lens && p.S > 0 && p.J > 0 && p.R0 > 0;
    return p.lens && !p.nsamp;
}

}  // namespace

hipError_t launch_sliding_assemble(const SlidingAssembleArgs &a, hipStream_t s) {
    if (!plan_ok(a.plan, false) || !a.feats || !a.lens || a.Bg <= 0 || a.i0 < 0 || a.F <= 0 || a.F % 4) return hipErrorInvalidValue;
    if (a.planes ? (!a.xh || !a.xl || a.Fp < a.F || a.Fp % 16 || a.tiles * SEQ_TILE < a.Bg) : (!a.out || a.flag)) return hipErrorInvalidValue;
    const long long rows = a.planes ? (long long)a.tiles * a.plan.W * SEQ_TILE : (long long)a.Bg * a.plan.W;
    const long long n = rows * ((a.planes ? a.Fp : a.F) / 4);
    hipLaunchKernelGGL(sliding_assemble_kernel, dim3(sliding_grid(n > a.Bg ? n : a.Bg, 4096)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sliding_wav_gather(const SlidingWavArgs &a, int is_i16, hipStream_t s) {
    if (!plan_ok(a.plan, true) || !a.pcm || !a.out || !a.nsamp_out || a.Bg <= 0 || a.Bg > 65535 || a.i0 < 0) return hipErrorInvalidValue;
    if (a.Sw != a.plan.R0 + a.plan.J * (long long)(a.plan.W - 1)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)sliding_grid(a.Sw, 4 + 4096 / a.Bg), (unsigned)a.Bg);
    if (is_i16) hipLaunchKernelGGL(sliding_wav_gather_kernel<int16_t>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sliding_wav_gather_kernel<float>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sliding_aggregate(const SlidingAggregateArgs &a, hipStream_t s) {
    if (!plan_ok(a.plan, a.plan.nsamp != nullptr) || !a.win || !a.out || a.ld_out < a.plan.T) return hipErrorInvalidValue;
    const dim3 grid((unsigned)sliding_grid(a.plan.T, 4 + 4096 / a.plan.nrec), (unsigned)a.plan.nrec);
    hipLaunchKernelGGL(sliding_aggregate_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
