// window_stream.hip -- the feature ring and window assembly of the windowed stream (uvad_window_step, include/uvad.h).
//
// A stream group of B feeds keeps, per feed, a ring of R >= W log-mel frames in its state: frame t lives in slot t % R.  Each step the
// feature kernel (fbank.hip, virtual [tail | chunk] rows) transforms only the k frames the chunk completes, into a small [B][k][F]
// buffer; window_assemble_kernel then
//   * reads e_prev (frames complete before the step) from the DEVICE counter ctr[parity], so that a graph captured around one
//     steady-state step replays correctly for any later one with the same launch arguments,
//   * writes the window [e - Tw, e) (e = e_prev + k) in order straight into the first projection's operand -- the (hi, lo) f16 planes
//     with tile-major K-blocked rows exactly as split_features_kernel (gemm_f16p.hip) writes them, or canonical f32 rows [B][Tw][F] --
//     taking the k new frames from the fbank buffer (and committing them to their ring slots) and the older ones from the ring,
//   * and stores e in ctr[parity ^ 1] for the next step.
// The slots of the new frames [e - k, e) and those of the older window frames [e - Tw, e - k) differ (Tw <= R), so no thread reads a
// slot another one writes.  window_emit_kernel copies the emitted frames' logits / probabilities out of the classifier's [B][Tw] rows.
#include "uvad_internal.h"

namespace uvad {

namespace {

__global__ __launch_bounds__(256) void window_assemble_kernel(WindowArgs a) {
    const long long e = a.ctr_in[0] + a.k;   // frames complete after this step
    const long long lo = e - a.Tw, e_new = e - a.k;
    if (a.ctr_out && blockIdx.x == 0 && threadIdx.x == 0) a.ctr_out[0] = e;
    const int q4 = (a.planes ? a.Fp : a.F) / 4;
    const long long rows = a.planes ? (long long)a.tiles * a.Tw * SEQ_TILE : (long long)a.B * a.Tw;
    const long long n = rows * q4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / q4;
        const int c = (int)(i - m * q4) * 4;
        int b, t;   // feed, window row
        if (a.planes) {
            const long long per_tile = (long long)a.Tw * SEQ_TILE;
            const int tile = (int)(m / per_tile);
            const int rem = (int)(m - (long long)tile * per_tile);
            t = rem / SEQ_TILE;
            b = tile * SEQ_TILE + (rem - t * SEQ_TILE);
        } else {
            b = (int)(m / a.Tw);
            t = (int)(m - (long long)b * a.Tw);
        }
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < a.B && c < a.F) {
            const long long f = lo + t;   // absolute frame index
            float *slot = a.ring + ((size_t)b * a.R + (size_t)(f % a.R)) * a.F + c;
            if (f >= e_new) {
                v = *reinterpret_cast<const float4 *>(a.newf + ((size_t)b * a.k + (size_t)(f - e_new)) * a.F + c);
                *reinterpret_cast<float4 *>(slot) = v;
            } else {
                v = *reinterpret_cast<const float4 *>(slot);
            }
        }
        if (!a.planes) {
            *reinterpret_cast<float4 *>(a.out + ((size_t)b * a.Tw + t) * a.F + c) = v;
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

__global__ __launch_bounds__(256) void window_emit_kernel(const float *logits_in, const float *probs_in, int B, int Tw, int r0, int n,
                                                          float *logits, float *probs, int ld_out) {
    const long long total = (long long)B * n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n), j = (int)(i - (long long)b * n);
        const size_t src = (size_t)b * Tw + r0 + j, dst = (size_t)b * ld_out + j;
        if (logits) logits[dst] = logits_in[src];
        if (probs) probs[dst] = probs_in[src];
    }
}

__global__ __launch_bounds__(64) void window_carry_kernel(const long long *ctr_in, long long *ctr_out) {
    if (threadIdx.x == 0) ctr_out[0] = ctr_in[0];
}

int grid_for(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace

hipError_t launch_window_assemble(const WindowArgs &a, hipStream_t s) {
    if (a.B <= 0 || a.Tw <= 0 || a.F <= 0 || a.F % 4 || a.R < a.Tw || a.k < 0 || a.k > a.Tw || !a.ring || !a.ctr_in) return hipErrorInvalidValue;
    if (a.k > 0 && !a.newf) return hipErrorInvalidValue;
    if (a.planes ? (!a.xh || !a.xl || a.Fp < a.F || a.Fp % 16 || a.tiles * SEQ_TILE < a.B) : !a.out) return hipErrorInvalidValue;
    const long long rows = a.planes ? (long long)a.tiles * a.Tw * SEQ_TILE : (long long)a.B * a.Tw;
    hipLaunchKernelGGL(window_assemble_kernel, dim3(grid_for(rows * ((a.planes ? a.Fp : a.F) / 4))), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_window_carry(const long long *ctr_in, long long *ctr_out, hipStream_t s) {
    if (!ctr_in || !ctr_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_carry_kernel, dim3(1), dim3(64), 0, s, ctr_in, ctr_out);
    return hipGetLastError();
}

hipError_t launch_window_emit(const float *logits_in, const float *probs_in, int B, int Tw, int r0, int n, float *logits, float *probs,
                              int ld_out, hipStream_t s) {
    if (B <= 0 || n <= 0) return hipSuccess;
    if (r0 < 0 || r0 + n > Tw || ld_out < n || (logits && !logits_in) || (probs && !probs_in)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_emit_kernel, dim3(grid_for((long long)B * n)), dim3(256), 0, s, logits_in, probs_in, B, Tw, r0, n, logits,
                       probs, ld_out);
    return hipGetLastError();
}

}  // namespace uvad
