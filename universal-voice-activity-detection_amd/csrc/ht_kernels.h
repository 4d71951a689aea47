// ht_kernels.h -- the training kernels that head_train.hip (uvad_head_train_*), lstm_train.hip (uvad_lstm_train_*) and sincnet_train.hip
// (uvad_sincnet_train_*) share: the valid mask, the exact-f32 tile GEMM ht_gemm_kernel<MODE> on v_mfma_f32_32x32x2_f32 with its segment
// partials, and the fold of the partials in segment order.  One copy of the source; each file that includes it compiles its own instances of
// the kernels it launches (they sit in an unnamed namespace), under that file's flags -- every includer builds with contraction off.
// A state is HeadTrainHeader | masters [Pp] | gradient accumulator [Pp] | m [Pp] | v [Pp] for every family; the header's magic word tells
// them apart.  The kernels that work on those blocks alone -- Adam, its commit, the read-out and the write -- are in optim.hip, once, behind
// launch_train_apply / _read / _write.  A kernel may also be handed a GUARD: three words somewhere in device memory (a workspace header) that
// must hold the values the launcher expects, or the kernel does nothing.
#pragma once
#include "uvad_internal.h"
#include "../../include/uvad.h"

#pragma clang fp contract(off)

namespace uvad {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int HT_TM = 64, HT_TN = 64, HT_KC = 32;
constexpr int HT_LD = 65;    // LDS row stride of a k-major tile: odd, so k-contiguous global rows scatter over the banks

__device__ __forceinline__ int ht_row_len(const int *lens, int b, int T) {
    if (!lens) return T;
    const int n = lens[b];
    return n < 0 ? 0 : n > T ? T : n;
}
__device__ __forceinline__ bool ht_state_ok(const void *state, unsigned magic, int P) {
    const HeadTrainHeader *hd = reinterpret_cast<const HeadTrainHeader *>(state);
    return hd->magic == magic && hd->P == P;
}
// the guard words of a launch (ptr == nullptr: none): a workspace header written by an earlier call must still say what this call assumes
struct HtGuard { const int *ptr; int w[3]; };
__device__ __forceinline__ bool ht_guard_ok(const HtGuard &g) {
    return !g.ptr || (g.ptr[0] == g.w[0] && g.ptr[1] == g.w[1] && g.ptr[2] == g.w[2]);
}


__global__ __launch_bounds__(256) void ht_valid_kernel(const int *lens, int B, int T, uint8_t *valid) {
    const int N = B * T;
    for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256) {
        const int b = n / T;
        valid[n] = (n - b * T) < ht_row_len(lens, b, T) ? 1 : 0;
    }
}

// C(m, n) = sum_k A(m, k) B(k, n) on a 64 x 64 tile; what m, n and k stand for depends on MODE:
//   0 forward          m frame, n unit o, k input i:    A = act_in [N][K] (k contiguous), B = W [o][i] (k contiguous)
//   1 backward data    m frame, n input i, k unit o:    A = d_l [N][K] (k contiguous), B = W [o][i] (n contiguous)
//   2 weight gradient  m unit o, n input i, k frame:    A = d_l [frame][M] (m contiguous), B = act_in [frame][Nc] (n contiguous);
//                      blockIdx.y is the segment, k runs over its frames
struct HtGemm {
    const float *A, *B; int M, Nc, K;        // extents of m, n and k (MODE 2: K = all frames)
    const uint8_t *a_valid;                  // MODE 0: rows of A that may be read (nullptr: all) -- A is x0
    const uint8_t *b_valid;                  // MODE 2: rows (frames) of B that may be read (nullptr: all) -- B is x0
    const float *bias; float slope;          // MODE 0 epilogue
    const float *act;                        // MODE 1 epilogue: the stored activation the factor is read from (nullptr: none), [M][Nc]
    const uint8_t *c_valid;                  // MODE 1: rows stored as +0 unless valid (nullptr: all stored as computed)
    float *C; long long ldc;                 // MODE 0 / 1: C [M][ldc]; MODE 2: the partial of segment z at C + z part_stride, [M][ldc]
    float *Cb;                               // MODE 2: the bias partial [M] of segment z at Cb + z part_stride
    long long part_stride; int seg;
    const void *state; unsigned magic; int P;   // operands inside the state are trusted only under its header
    HtGuard guard;                           // ... and those inside a workspace only under its guard words
    int c_add;                               // MODE 1: the product is ADDED to what C holds (the second direction's share of one sum)
};

template <int MODE>
__global__ __launch_bounds__(256) void ht_gemm_kernel(HtGemm g) {
    __shared__ float As[HT_KC * HT_LD], Bs[HT_KC * HT_LD];
    if (!ht_state_ok(g.state, g.magic, g.P) || !ht_guard_ok(g.guard)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_n = (g.Nc + HT_TN - 1) / HT_TN;
    const int m0 = (int)(blockIdx.x / (unsigned)tiles_n) * HT_TM, n0 = (int)(blockIdx.x % (unsigned)tiles_n) * HT_TN;
    int kb = 0, ke = g.K;
    if (MODE == 2) {
        kb = (int)blockIdx.y * g.seg;
        ke = kb + g.seg < g.K ? kb + g.seg : g.K;
    }
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    // MODE 0 / 1: acc is the one chain over K.  MODE 2: acc is the chain over one 32-frame chunk and tot the chunk sums added in chunk order,
    // the bias partial's two short chains: one chain over a whole default segment of 2048 frames measured 2 x torch's f32 rms error on the
    // LSTM's weight_ih gradients at N = 3000 and 4.1 x its max error.  A segment of one chunk gives the bits it always gave (tot = +0 + acc).
    f32x16 acc, tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.0f; tot[r] = 0.0f; }
    float bsum = 0.0f;                       // MODE 2, n-tile 0, tid < 64: the bias partial of unit m0 + tid
    for (int k0 = kb; k0 < ke; k0 += HT_KC) {
        // stage A and B, k-major: As[k][m], Bs[k][n]; everything outside the operands is zero and never read
#pragma unroll
        for (int i = 0; i < HT_TM * HT_KC / 256; ++i) {
            const int e = tid + 256 * i;
            int mm, kk;
            if (MODE == 2) { mm = e % HT_TM; kk = e / HT_TM; } else { kk = e % HT_KC; mm = e / HT_KC; }
            const int m = m0 + mm, k = k0 + kk;
            float v = 0.0f;
            if (m < g.M && k < ke) {
                if (MODE == 2) v = g.A[(size_t)k * g.M + m];
                else if (MODE == 1 || !g.a_valid || g.a_valid[m]) v = g.A[(size_t)m * g.K + k];
            }
            As[kk * HT_LD + mm] = v;
        }
#pragma unroll
        for (int i = 0; i < HT_TN * HT_KC / 256; ++i) {
            const int e = tid + 256 * i;
            int nn, kk;
            if (MODE == 0) { kk = e % HT_KC; nn = e / HT_KC; } else { nn = e % HT_TN; kk = e / HT_TN; }
            const int n = n0 + nn, k = k0 + kk;
            float v = 0.0f;
            if (n < g.Nc && k < ke) {
                if (MODE == 0) v = g.B[(size_t)n * g.K + k];
                else if (MODE == 1 || !g.b_valid || g.b_valid[k]) v = g.B[(size_t)k * g.Nc + n];
            }
            Bs[kk * HT_LD + nn] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < HT_KC; kk += 2) {
            const float a = As[(kk + (lane >> 5)) * HT_LD + wm + (lane & 31)];
            const float b = Bs[(kk + (lane >> 5)) * HT_LD + wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        if (MODE == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { tot[r] = tot[r] + acc[r]; acc[r] = 0.0f; }
        }
        if (MODE == 2 && n0 == 0 && tid < HT_TM) {   // the chunk's 32 frames in order (zeros past the segment), then the chunks in order: two short
            float c = 0.0f;                            // chains (32 and segment / 32 terms), not one of `segment` terms whose error grows with its length
#pragma unroll
            for (int kk = 0; kk < HT_KC; ++kk) c += As[kk * HT_LD + tid];
            bsum += c;
        }
        __syncthreads();
    }
    // C / D map of the 32 x 32 shapes: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float *C = MODE == 2 ? g.C + (size_t)blockIdx.y * g.part_stride : g.C;
    const int n = n0 + wn + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.M || n >= g.Nc) continue;
        float v = MODE == 2 ? tot[r] : acc[r];
        if (MODE == 0) {
            v = v + g.bias[n];
            v = v > 0.0f ? v : v * g.slope;
        } else if (MODE == 1) {
            if (g.c_add) v = C[(size_t)m * g.ldc + n] + v;
            if (g.act) v = v * (g.act[(size_t)m * g.Nc + n] > 0.0f ? 1.0f : g.slope);
            if (g.c_valid && !g.c_valid[m]) v = 0.0f;
        }
        C[(size_t)m * g.ldc + n] = v;
    }
    if (MODE == 2 && n0 == 0 && tid < HT_TM && m0 + tid < g.M) g.Cb[(size_t)blockIdx.y * g.part_stride + m0 + tid] = bsum;
}

// acc[j] += the partials of parameter j in segment order; workgroup 0 also folds the loss partials and the frame count
__global__ __launch_bounds__(256) void ht_fold_kernel(void *state, unsigned magic, int P, int Pp, const float *part, int nseg, const double *loss_part,
                                                      int nloss, int count_loss, const int *lens, int B, int T, HeadTrainWsHead *head, HtGuard guard) {
    __shared__ double lsh[256];
    __shared__ unsigned long long vsh[256];
    if (!ht_state_ok(state, magic, P) || !ht_guard_ok(guard)) return;
    HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(state);
    float *acc = reinterpret_cast<float *>(hd + 1) + Pp;
    const int tid = threadIdx.x;
    const int j = (int)blockIdx.x * 256 + tid;
    if (j < P) {
        float s = part[j];
        for (int z = 1; z < nseg; ++z) s = s + part[(size_t)z * Pp + j];
        acc[j] = acc[j] + s;
    }
    if (blockIdx.x != 0) return;
    double l = 0.0;
    unsigned long long valid = 0ull;
    if (count_loss)
        for (int i = tid; i < nloss; i += 256) l += loss_part[i];
    for (int b = tid; b < B; b += 256) valid += (unsigned long long)ht_row_len(lens, b, T);
    lsh[tid] = l;
    vsh[tid] = valid;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) { lsh[tid] += lsh[tid + o]; vsh[tid] += vsh[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        head->loss = lsh[0];
        head->frames = vsh[0];
        hd->loss += lsh[0];
        hd->frames += vsh[0];
    }
}

inline size_t ht_align(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace
}  // namespace uvad
