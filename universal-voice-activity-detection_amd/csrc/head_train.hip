// head_train.hip -- fine-tuning of the head (uvad_head_train_*, include/uvad.h): the feed-forward layers and the classifier learn on top
// of the frozen LSTM output x0 [B][T][D0]; what VadModel.training_step / configure_optimizers of src/engines/vad_engine.py do for that
// slice of the model (F.leaky_relu(linear(x)), F.binary_cross_entropy with the mean over the frames present, torch.optim.Adam).
//
// Frames are flat (n = b T + t, N = B T).  The three contraction families run on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: a
// k-ordered fma chain, bit for bit) through ONE tile kernel, ht_gemm_kernel<MODE>: a 64 x 64 output tile per workgroup, one 32 x 32
// quadrant per wave, both operands staged through LDS k-major in chunks of 32 so that the fragment reads are conflict-free whichever way
// the operand lies in memory.  The masters are plain f32 in torch layout: no transposed copy, the backward-data product reads the
// weight in the other operand order.
//   ht_valid_kernel       valid[n] = t < len_b, one byte per frame: what every later kernel selects with (frames past a length are never
//                         read in x0, the labels, the weights or a caller's dz)
//   ht_gemm_kernel<0>     a_l = leaky_relu(a_{l-1} W_l^T + b_l), kept in the workspace
//   ht_cls_kernel         z = a_L . w_c + b_c, p = sigmoid(z), the loss terms in f64 and dz, one wave per frame; a loss partial per 256 frames
//   ht_dlast_kernel       d_L = (dz w_c) * leaky'(a_L), or for a head without feed-forward layers d_grad_x = dz w_c
//   ht_gemm_kernel<2>     dW_l = sum_n d_l[n][o] a_{l-1}[n][i] and db_l = sum_n d_l[n][o] (both as 32-frame chunk sums, added in order) over one
//                         segment of frames: a partial in the workspace
//   ht_gemm_kernel<1>     d_{l-1} = (d_l W_l) * leaky'(a_{l-1}); the last one is d_grad_x (no factor, +0 past the lengths)
//   ht_fold_kernel        the partials in segment order into the accumulator, the loss partials and the frame count into the state: no
//                         floating-point atomics anywhere, the same calls give the same bits
//   ht_reset_kernel       the state from the context's head tensors
// The Adam step, the read-out and the write work on the state's blocks alone and serve every family: launch_train_apply / _read / _write
// of optim.hip.
// Contraction is off in the whole file (#pragma clang fp contract(off) in ht_kernels.h and the Makefile's flag): the elementwise arithmetic
// is restated operation by operation on the CPU, and the matrix instruction is not affected.
// ht_valid_kernel, ht_gemm_kernel (its products are __builtin_amdgcn_mfma_f32_32x32x2f32) and ht_fold_kernel live in ht_kernels.h, which
// lstm_train.hip (uvad_lstm_train_*: the backward pass d_grad_x starts) and sincnet_train.hip include as well.
#include "ht_kernels.h"

namespace uvad {

static_assert(sizeof(HeadTrainHeader) == 256 && sizeof(HeadTrainWsHead) == 256, "state and workspace layout");
static_assert(HT_SCALAR_WORDS == UVAD_HEAD_TRAIN_SCALAR_WORDS, "the scalar record of include/uvad.h");

namespace {

struct HtCls {
    const float *a; int K;                   // the classifier's input rows [N][K] (x0 when the head has no feed-forward layer)
    const uint8_t *valid; int x_is_input;    // x_is_input: rows of `a` are read only where valid
    const float *wc, *bc;
    const uint8_t *gt; int ld_gt; const float *fw; int ld_fw; const float *dz_in; int ld_dz;
    float *probs; int ld_p;
    float *dz; double *loss_part;
    int N, T;
    const void *state; int P;
};

// one workgroup per HT_LOSS_BLOCK frames, a wave per 64 of them: the dot product of one frame at a time across the lanes (a fixed tree),
// then lane j finishes frame j
__global__ __launch_bounds__(256) void ht_cls_kernel(HtCls a) {
    __shared__ double lsh[4];
    if (!ht_state_ok(a.state, HT_MAGIC, a.P)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = (int)blockIdx.x * HT_LOSS_BLOCK + wave * 64;
    const float bc = a.bc[0];
    float z = 0.0f;
    for (int j = 0; j < 64; ++j) {
        const int n = f0 + j;
        if (n >= a.N) break;                                     // wave-uniform
        if (a.x_is_input && !a.valid[n]) continue;               // wave-uniform: the row is never read
        const float *row = a.a + (size_t)n * a.K;
        float s = 0.0f;
        for (int k = lane; k < a.K; k += 64) s = s + row[k] * a.wc[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o);
        if (lane == j) z = s + bc;
    }
    const int n = f0 + lane;
    double term = 0.0;
    if (n < a.N) {
        float dz = 0.0f;
        if (a.valid[n]) {
            const int b = n / a.T, t = n - b * a.T;
            const float p = 1.0f / (1.0f + expf(-z));            // head.hip's sigmoid
            if (a.probs) a.probs[(size_t)b * a.ld_p + t] = p;
            if (a.dz_in) {
                dz = a.dz_in[(size_t)b * a.ld_dz + t];
            } else {
                const bool y = a.gt[(size_t)b * a.ld_gt + t] != 0;
                const float w = a.fw ? a.fw[(size_t)b * a.ld_fw + t] : 1.0f;
                const double q1 = y ? (double)p : 1.0 - (double)p;   // exact: p is an f32
                double l = log(q1);
                if (l < -100.0) l = -100.0;                      // F.binary_cross_entropy's clamp
                term = (double)w * -l;
                // what autograd gives for BCE on sigmoid(z): each operation rounded once, in this order
                const float d = p - (y ? 1.0f : 0.0f);
                const float q = p * (1.0f - p);
                const float qm = q > 1e-12f ? q : 1e-12f;
                dz = w * (d * (q / qm));                         // q / qm is exactly 1 unless p (1 - p) < 1e-12: dz = w (p - y)
            }
        }
        a.dz[n] = dz;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) term += __shfl_xor(term, o);   // a fixed tree
    if (lane == 0) lsh[wave] = term;
    __syncthreads();
    if (tid == 0) a.loss_part[blockIdx.x] = ((lsh[0] + lsh[1]) + lsh[2]) + lsh[3];
}

// out[n][i] = (dz[n] wc[i]) * leaky'(act[n][i]) (act == nullptr: no factor); rows past a length are +0
__global__ __launch_bounds__(256) void ht_dlast_kernel(const float *dz, const float *wc, const float *act, const uint8_t *valid, float slope,
                                                       float *out, int N, int K, const void *state, int P) {
    if (!ht_state_ok(state, HT_MAGIC, P)) return;
    const size_t total = (size_t)N * K;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int n = (int)(e / K), i = (int)(e - (size_t)n * K);
        float v = 0.0f;
        if (valid[n]) {
            v = dz[n] * wc[i];
            if (act) v = v * (act[e] > 0.0f ? 1.0f : slope);
        }
        out[e] = v;
    }
}

__global__ __launch_bounds__(256) void ht_reset_kernel(HeadTrainShape q, HeadTrainInit in, void *state) {
    HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(state);
    float *w = reinterpret_cast<float *>(hd + 1);
    const int gtid = (int)blockIdx.x * 256 + threadIdx.x, gsz = (int)gridDim.x * 256;
    for (int j = gtid; j < 4 * q.Pp; j += gsz) {
        float v = 0.0f;
        if (j < q.P) {
            int l = 0;
            while (l < q.L && j >= q.off_w[l + 1]) ++l;          // the tensor pair (weight, bias) j belongs to
            if (j >= q.off_b[l]) v = in.b[l][j - q.off_b[l]];
            else {
                const int K = l == q.L ? (q.L ? q.H : q.D0) : (l ? q.H : q.D0);
                const int e = j - q.off_w[l];
                v = in.w[l][(size_t)(e / K) * in.ldw[l] + e % K];
            }
        }
        w[j] = v;
    }
    if (gtid == 0) {
        HeadTrainHeader h{};
        h.magic = HT_MAGIC; h.D0 = q.D0; h.H = q.H; h.L = q.L; h.P = q.P;
        h.loss = 0.0; h.frames = 0ull; h.t = 0ull; h.bc1 = 0.0f; h.bc2 = 0.0f;
        *hd = h;
    }
}

}  // namespace

HeadTrainShape head_train_shape(int D0, int H, int L, float slope) {
    HeadTrainShape q{};
    q.D0 = D0; q.H = H; q.L = L; q.slope = slope;
    int off = 0, K = D0;
    for (int l = 0; l < L; ++l) {
        q.off_w[l] = off; off += H * K;
        q.off_b[l] = off; off += H;
        K = H;
    }
    q.off_w[L] = off; off += K;
    q.off_b[L] = off; off += 1;
    for (int l = L + 1; l <= HT_MAX_LAYERS; ++l) q.off_w[l] = q.off_b[l] = off;
    q.P = off;
    q.Pp = (off + 63) / 64 * 64;
    return q;
}

size_t head_train_state_bytes(const HeadTrainShape &q) { return sizeof(HeadTrainHeader) + (size_t)4 * q.Pp * sizeof(float); }

HeadTrainWs head_train_ws(const HeadTrainShape &q, long long N, int seg) {
    HeadTrainWs w{};
    w.N = (int)N;
    w.nseg = (int)((N + seg - 1) / seg);
    size_t off = sizeof(HeadTrainWsHead);
    w.off_valid = off; off = ht_align(off + (size_t)N);
    w.off_dz = off; off = ht_align(off + (size_t)N * sizeof(float));
    w.off_act = off; off = ht_align(off + (size_t)q.L * N * q.H * sizeof(float));
    for (int i = 0; i < 2; ++i) { w.off_d[i] = off; off = ht_align(off + (q.L ? (size_t)N * q.H * sizeof(float) : 0)); }
    w.off_part = off; off = ht_align(off + (size_t)w.nseg * q.Pp * sizeof(float));
    w.off_loss = off; off = ht_align(off + (size_t)((N + HT_LOSS_BLOCK - 1) / HT_LOSS_BLOCK) * sizeof(double));
    w.total = off;
    return w;
}

hipError_t launch_head_train_reset(const HeadTrainShape &q, const HeadTrainInit &in, void *state, hipStream_t s) {
    if (!state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ht_reset_kernel, dim3(64), dim3(256), 0, s, q, in, state);
    return hipGetLastError();
}

hipError_t launch_head_train_grad(const HeadTrainShape &q, const HeadTrainGradArgs &a, hipStream_t s) {
    if (!a.x || !a.state || !a.ws || a.B <= 0 || a.T <= 0 || (long long)a.B * a.T > HT_MAX_FRAMES || a.seg < HT_MIN_SEGMENT ||
        a.seg > HT_MAX_SEGMENT || a.seg % 32 || (!a.dz_in && !a.gt) || q.L < 0 || q.L > HT_MAX_LAYERS)
        return hipErrorInvalidValue;
    const int N = a.B * a.T, H = q.H, L = q.L;
    const HeadTrainWs w = head_train_ws(q, N, a.seg);
    char *base = reinterpret_cast<char *>(a.ws);
    uint8_t *valid = reinterpret_cast<uint8_t *>(base + w.off_valid);
    float *dz = reinterpret_cast<float *>(base + w.off_dz);
    float *act = reinterpret_cast<float *>(base + w.off_act);
    float *dbuf[2] = {reinterpret_cast<float *>(base + w.off_d[0]), reinterpret_cast<float *>(base + w.off_d[1])};
    float *part = reinterpret_cast<float *>(base + w.off_part);
    double *loss_part = reinterpret_cast<double *>(base + w.off_loss);
    const float *master = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.state) + sizeof(HeadTrainHeader));
    auto act_of = [&](int l) -> const float * { return l == 0 ? a.x : act + (size_t)(l - 1) * N * H; };   // a_l, l = 0 .. L
    auto width_of = [&](int l) { return l == 0 ? q.D0 : H; };
    auto tiles = [](int M, int Nc) { return (unsigned)(((M + HT_TM - 1) / HT_TM) * ((Nc + HT_TN - 1) / HT_TN)); };
    hipError_t e;
#define HT_LAUNCHED() do { e = hipGetLastError(); if (e != hipSuccess) return e; } while (0)

    hipLaunchKernelGGL(ht_valid_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a.lens, a.B, a.T, valid);
    HT_LAUNCHED();
    for (int l = 1; l <= L; ++l) {   // a_l = leaky_relu(a_{l-1} W_l^T + b_l)
        HtGemm g{};
        g.A = act_of(l - 1); g.B = master + q.off_w[l - 1]; g.M = N; g.Nc = H; g.K = width_of(l - 1);
        g.a_valid = l == 1 ? valid : nullptr;
        g.bias = master + q.off_b[l - 1]; g.slope = q.slope;
        g.C = act + (size_t)(l - 1) * N * H; g.ldc = H;
        g.state = a.state; g.magic = HT_MAGIC; g.P = q.P;
        hipLaunchKernelGGL(ht_gemm_kernel<0>, dim3(tiles(N, H)), dim3(256), 0, s, g);
        HT_LAUNCHED();
    }
    const int KL = width_of(L);
    {
        HtCls c{};
        c.a = act_of(L); c.K = KL; c.valid = valid; c.x_is_input = L == 0;
        c.wc = master + q.off_w[L]; c.bc = master + q.off_b[L];
        c.gt = a.gt; c.ld_gt = a.ld_gt; c.fw = a.fw; c.ld_fw = a.ld_fw; c.dz_in = a.dz_in; c.ld_dz = a.ld_dz;
        c.probs = a.probs; c.ld_p = a.ld_p; c.dz = dz; c.loss_part = loss_part; c.N = N; c.T = a.T;
        c.state = a.state; c.P = q.P;
        hipLaunchKernelGGL(ht_cls_kernel, dim3((unsigned)((N + HT_LOSS_BLOCK - 1) / HT_LOSS_BLOCK)), dim3(256), 0, s, c);
        HT_LAUNCHED();
    }
    {   // the classifier's gradients: dw_c = sum_n dz[n] a_L[n][:], db_c = sum_n dz[n]
        HtGemm g{};
        g.A = dz; g.B = act_of(L); g.M = 1; g.Nc = KL; g.K = N; g.b_valid = L == 0 ? valid : nullptr;
        g.C = part + q.off_w[L]; g.ldc = KL; g.Cb = part + q.off_b[L]; g.part_stride = q.Pp; g.seg = a.seg;
        g.state = a.state; g.magic = HT_MAGIC; g.P = q.P;
        hipLaunchKernelGGL(ht_gemm_kernel<2>, dim3(tiles(1, KL), (unsigned)w.nseg), dim3(256), 0, s, g);
        HT_LAUNCHED();
    }
    if (L > 0 || a.grad_x) {   // d_L, or d_grad_x of a head without feed-forward layers
        float *out = L > 0 ? dbuf[L & 1] : a.grad_x;
        const size_t total = (size_t)N * KL;
        const unsigned blocks = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
        hipLaunchKernelGGL(ht_dlast_kernel, dim3(blocks), dim3(256), 0, s, dz, master + q.off_w[L], L > 0 ? act_of(L) : nullptr, valid, q.slope,
                           out, N, KL, a.state, q.P);
        HT_LAUNCHED();
    }
    for (int l = L; l >= 1; --l) {
        const float *d = dbuf[l & 1];
        const int K = width_of(l - 1);
        {   // dW_l = sum_n d_l[n][o] a_{l-1}[n][i], db_l = sum_n d_l[n][o]
            HtGemm g{};
            g.A = d; g.B = act_of(l - 1); g.M = H; g.Nc = K; g.K = N; g.b_valid = l == 1 ? valid : nullptr;
            g.C = part + q.off_w[l - 1]; g.ldc = K; g.Cb = part + q.off_b[l - 1]; g.part_stride = q.Pp; g.seg = a.seg;
            g.state = a.state; g.magic = HT_MAGIC; g.P = q.P;
            hipLaunchKernelGGL(ht_gemm_kernel<2>, dim3(tiles(H, K), (unsigned)w.nseg), dim3(256), 0, s, g);
            HT_LAUNCHED();
        }
        if (l > 1 || a.grad_x) {   // d_{l-1} = (d_l W_l) * leaky'(a_{l-1}); the last one is d_grad_x
            HtGemm g{};
            g.A = d; g.B = master + q.off_w[l - 1]; g.M = N; g.Nc = K; g.K = H;
            g.act = l > 1 ? act_of(l - 1) : nullptr; g.slope = q.slope;
            g.c_valid = l == 1 ? valid : nullptr;
            g.C = l > 1 ? dbuf[(l - 1) & 1] : a.grad_x; g.ldc = K;
            g.state = a.state; g.magic = HT_MAGIC; g.P = q.P;
            hipLaunchKernelGGL(ht_gemm_kernel<1>, dim3(tiles(N, K)), dim3(256), 0, s, g);
            HT_LAUNCHED();
        }
    }
    hipLaunchKernelGGL(ht_fold_kernel, dim3((unsigned)((q.P + 255) / 256)), dim3(256), 0, s, a.state, HT_MAGIC, q.P, q.Pp, part, w.nseg,
                       loss_part, (N + HT_LOSS_BLOCK - 1) / HT_LOSS_BLOCK, a.dz_in ? 0 : 1, a.lens, a.B, a.T, reinterpret_cast<HeadTrainWsHead *>(base),
                       HtGuard{});
    HT_LAUNCHED();
#undef HT_LAUNCHED
    return hipSuccess;
}

}  // namespace uvad
