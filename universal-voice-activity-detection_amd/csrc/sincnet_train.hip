// sincnet_train.hip -- training of the SincNet front end (uvad_sincnet_train_*, include/uvad.h): the forward pass with kept activations from
// the STATE's f32 masters, autograd's backward pass through wav_norm1d, the parameterised sinc bank, |.| and the three (conv, MaxPool1d(3),
// InstanceNorm1d, leaky_relu) stages of src/models/blocks/sincnet.py, and torch.optim.Adam on their tensors.  Dense batches: B rows of S samples.
//
// Stage s has Cin / Cout channels, Kw taps, L conv positions and Lp = L / 3 pooled positions; the conv positions past 3 Lp take part in nothing.
// Forward:
//   st_bank_kernel        the n_filters x kernel_size bank from low_hz_ / band_hz_ as ParamSincFB.filters() defines it, in double, rounded once
//                         (a frozen stage 0 whose state has no band edges runs the bank that reset copied in)
//   st_wav_stats_kernel   per row: biased variance, scale / shift of wav_norm1d and the pair that gives the normalised row; the workspace header
//   st_conv_kernel        u = conv(a_in) (+ bias), |u| for stage 0, p = max of three, the LOWEST index winning a tie: an implicit GEMM on
//                         v_mfma_f32_32x32x2_f32 (m = out channel, n = pooled position, k = (in channel, tap)) with one accumulator per pool
//                         phase, so the pool is elementwise in registers.  The B staging reads the Hankel window of the stage's input, which
//                         it recomputes from the stage below: x scale + shift for the waveform, leaky_relu(gamma xhat + beta) above.
//                         Keeps p and one byte per pooled element: winner in bits 0 .. 1, stage 0's sign of the winning conv output in bits
//                         2 .. 3 (1: > 0, 2: < 0, 0: +-0).  The pre-pool conv output is not kept.
//   st_stats_kernel       mean and rstd per (b, c) over the pooled positions: one wave, two passes in double, lanes folded in a fixed order
//   st_out_kernel         feats [B][T][c3] = the last stage's leaky_relu(gamma xhat + beta)
// Backward, stages 2 .. first_stage:
//   st_norm_bwd_kernel    one wave per (b, c): dz = d_a_out leaky'(z), the four row sums in double, then
//                         dp = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), times the kept sign for stage 0; per-row shares of d gamma, d beta
//   st_cfold_kernel       d gamma, d beta: the rows' shares added in row order
//   st_wgrad_kernel       dW (stage 0: G, the same contraction against the normalised row) and d bias (stage 0: D) per segment of `segment`
//                         flat conv positions (b 3 Lp + t): ht_gemm_kernel<2>'s shape, m = out channel, n = (in channel, tap), k = position.
//                         The PLAIN form: k runs over conv positions, the A staging forms du[3 l + winner] = dp from the pooled gradient and
//                         the winner byte (du itself is never stored), the B staging computes the Hankel address.
//   st_dgrad_kernel       d_a_in[ci][j] = sum_{co, tap} du[co][j - tap] W[co][ci][tap]: m = in channel, n = position, k = (out channel, tap)
//   st_gfold_kernel, st_bank_bwd_kernel   stage 0: G and D folded in segment order, dF = g G + b0 D, d g = sum F G, d b0 = sum_c D_c sum_k F_ck,
//                         and d low_hz_ / d band_hz_ by the chain rule through filters() in double
//   ht_fold_kernel        as the head's; Adam, the read-out and the write are launch_train_apply / _read / _write of optim.hip
// No floating-point atomics; every reduction has a fixed order, so the same calls give the same bits.  Every backward kernel checks the state's
// and the workspace's headers on the device and writes nothing under a mismatch.  Contraction is off; the fused multiply-adds are explicit.
#include "ht_kernels.h"

namespace uvad {

static_assert(sizeof(SincTrainWsHead) == 256, "workspace layout");

namespace {

constexpr int ST_PT = 64;                 // pooled positions per conv tile
constexpr int ST_LB = 3 * ST_PT + 1;      // LDS row stride of the conv B tile: 192 conv positions, odd
constexpr double ST_MIN_LOW = 50.0, ST_MIN_BAND = 50.0, ST_RATE = 16000.0;   // ParamSincFB as SincNet builds it

// z of a pooled value under the norm of its stage; xhat on the way
__device__ __forceinline__ float st_z(float p, float mean, float rstd, float gamma, float beta, float &xhat) {
    xhat = (p - mean) * rstd;
    return gamma * xhat + beta;
}
__device__ __forceinline__ float st_leaky(float z, float slope) { return z > 0.0f ? z : z * slope; }

// the input of a stage as its contractions read it
struct StIn {
    const float *x;              // stage 0: the waveform [B][S]; above: the pooled values of the stage below [B][Cin][Lin]
    const float *stat;           // stage 0: [B][4] {scale, shift, rstd, -mean rstd}; above: [B][Cin][2] {mean, rstd}
    const float *gamma, *beta;   // above stage 0: the norm of the stage below
    long long bstride;           // S, or Cin Lin
    int Cin, Lin;
    float slope;
};
// S0: the waveform through wav_norm1d (HAT: the normalised row before the affine)
template <bool S0, bool HAT>
__device__ __forceinline__ float st_in(const StIn &a, int b, int ci, long long pos) {
    if (S0) {
        const float *st = a.stat + (size_t)b * 4 + (HAT ? 2 : 0);
        return __builtin_fmaf(a.x[(size_t)b * a.bstride + pos], st[0], st[1]);
    }
    const float *st = a.stat + ((size_t)b * a.Cin + ci) * 2;
    float xh;
    return st_leaky(st_z(a.x[(size_t)b * a.bstride + (size_t)ci * a.Lin + pos], st[0], st[1], a.gamma[ci], a.beta[ci], xh), a.slope);
}

// du[co][t] of row b from the pooled gradient and the winner byte; t < 3 Lp
__device__ __forceinline__ float st_du(const float *dp, const uint8_t *idx, int b, int Cout, int Lp, int co, int t) {
    const int l = t / 3, r = t - 3 * l;
    const size_t o = ((size_t)b * Cout + co) * Lp + l;
    return (idx[o] & 3) == r ? dp[o] : 0.0f;
}

struct StBank {
    const float *low, *band, *win, *nn;   // [NF / 2], [NF / 2], [half], [half]
    float *bank; int NF, KS;              // [NF][KS]
    const void *state; int P;
};
struct StEdges { double low, high, bandw; bool pass; };
__device__ __forceinline__ StEdges st_edges(float lp, float bp) {
    StEdges e;
    e.low = ST_MIN_LOW + fabs((double)lp);
    const double raw = e.low + ST_MIN_BAND + fabs((double)bp);
    e.pass = raw >= ST_MIN_LOW && raw <= ST_RATE / 2;
    e.high = raw < ST_MIN_LOW ? ST_MIN_LOW : raw > ST_RATE / 2 ? ST_RATE / 2 : raw;
    e.bandw = e.high - e.low;
    return e;
}

__global__ __launch_bounds__(256) void st_bank_kernel(StBank a) {
    if (!ht_state_ok(a.state, SNT_MAGIC, a.P)) return;
    if (!reinterpret_cast<const HeadTrainHeader *>(a.state)->pad0) return;   // reset found no band edges: the bank it copied in stays
    const int half = a.KS / 2, cut = a.NF / 2;
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (e >= cut * half) return;
    const int c = e / half, i = e - c * half;
    const StEdges q = st_edges(a.low[c], a.band[c]);
    const double n = (double)a.nn[i], w = (double)a.win[i];
    const double fl = q.low * n, fh = q.high * n;
    const double cl = ((sin(fh) - sin(fl)) / (n / 2)) * w / (2 * q.bandw);
    const double sl = ((cos(fl) - cos(fh)) / (n / 2)) * w / (2 * q.bandw);
    float *fc = a.bank + (size_t)c * a.KS, *fs = a.bank + (size_t)(c + cut) * a.KS;
    fc[i] = (float)cl; fc[a.KS - 1 - i] = (float)cl;
    fs[i] = (float)sl; fs[a.KS - 1 - i] = (float)(-sl);
    if (i == 0) { fc[half] = (float)((2 * q.bandw) / (2 * q.bandw)); fs[half] = 0.0f; }
}

__global__ __launch_bounds__(256) void st_wav_stats_kernel(const float *wav, int B, long long S, const float *gamma, const float *beta, float eps,
                                                           float *wstat, SincTrainWsHead *head, const void *state, int P) {
    __shared__ double red[2][4];
    if (!ht_state_ok(state, SNT_MAGIC, P)) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *x = wav + (size_t)b * S;
    double s = 0.0, ss = 0.0;
    for (long long i = tid; i < S; i += 256) {
        const double v = x[i];
        s += v;
        ss += v * v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = ss; }
    __syncthreads();
    if (tid == 0) {
        s = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        ss = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        const double mean = s / (double)S;
        double var = ss / (double)S - mean * mean;
        if (var < 0.0) var = 0.0;
        const double rstd = 1.0 / sqrt(var + (double)eps), sc = (double)gamma[0] * rstd;
        float *o = wstat + (size_t)b * 4;
        o[0] = (float)sc;
        o[1] = (float)((double)beta[0] - mean * sc);
        o[2] = (float)rstd;
        o[3] = (float)(-mean * rstd);
        if (b == 0) { head->magic = SNT_WS_MAGIC ^ (int)(S >> 32); head->B = B; head->S_lo = (int)S; head->S_hi = (int)(S >> 32); }
    }
}

struct StConv {
    StIn in;
    const float *W, *bias;       // W [Cout][K], k = ci Kw + tap; bias [Cout] or nullptr (the sinc bank has none)
    int Cout, K, Kw, stride, Lp;
    float *p; uint8_t *idx;      // [B][Cout][Lp]
    const void *state; int P;
};

template <bool S0>
__global__ __launch_bounds__(256) void st_conv_kernel(StConv g) {
    __shared__ float As[HT_KC * HT_LD], Bs[HT_KC * ST_LB];
    if (!ht_state_ok(g.state, SNT_MAGIC, g.P)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int tiles_n = (g.Lp + ST_PT - 1) / ST_PT;
    const int m0 = (int)(blockIdx.x / (unsigned)tiles_n) * HT_TM, lp0 = (int)(blockIdx.x % (unsigned)tiles_n) * ST_PT;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x16 acc0, acc1, acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; acc2[r] = 0.0f; }
    for (int k0 = 0; k0 < g.K; k0 += HT_KC) {
#pragma unroll
        for (int i = 0; i < HT_TM * HT_KC / 256; ++i) {
            const int e = tid + 256 * i, kk = e % HT_KC, mm = e / HT_KC;
            const int m = m0 + mm, k = k0 + kk;
            As[kk * HT_LD + mm] = m < g.Cout && k < g.K ? g.W[(size_t)m * g.K + k] : 0.0f;
        }
#pragma unroll 4
        for (int i = 0; i < 3 * ST_PT * HT_KC / 256; ++i) {
            const int e = tid + 256 * i, j = e % (3 * ST_PT), kk = e / (3 * ST_PT);
            const int k = k0 + kk, pos = 3 * lp0 + j;
            float v = 0.0f;
            if (k < g.K && pos < 3 * g.Lp) {
                const int ci = k / g.Kw, tap = k - ci * g.Kw;
                v = st_in<S0, false>(g.in, b, ci, (long long)pos * g.stride + tap);
            }
            Bs[kk * ST_LB + j] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < HT_KC; kk += 2) {
            const float a = As[(kk + (lane >> 5)) * HT_LD + wm + (lane & 31)];
            const float *br = &Bs[(kk + (lane >> 5)) * ST_LB + 3 * (wn + (lane & 31))];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, br[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, br[1], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, br[2], acc2, 0, 0, 0);
        }
        __syncthreads();
    }
    const int lp = lp0 + wn + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.Cout || lp >= g.Lp) continue;
        float u0 = acc0[r], u1 = acc1[r], u2 = acc2[r];
        if (!S0) {
            const float bv = g.bias[m];
            u0 = u0 + bv; u1 = u1 + bv; u2 = u2 + bv;
        }
        const float v0 = S0 ? __builtin_fabsf(u0) : u0, v1 = S0 ? __builtin_fabsf(u1) : u1, v2 = S0 ? __builtin_fabsf(u2) : u2;
        float pv = v0, uw = u0;
        int w = 0;
        if (v1 > pv) { pv = v1; uw = u1; w = 1; }
        if (v2 > pv) { pv = v2; uw = u2; w = 2; }
        if (S0) w |= uw > 0.0f ? 4 : uw < 0.0f ? 8 : 0;
        const size_t o = ((size_t)b * g.Cout + m) * g.Lp + lp;
        g.p[o] = pv;
        g.idx[o] = (uint8_t)w;
    }
}

// one wave per (b, c): the mean in double, then the squares about it
__global__ __launch_bounds__(64) void st_stats_kernel(const float *p, int Lp, float eps, float *stat, const void *state, int P) {
    if (!ht_state_ok(state, SNT_MAGIC, P)) return;
    const size_t row = blockIdx.x;
    const float *x = p + row * Lp;
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int l = lane; l < Lp; l += 64) s += (double)x[l];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    const double mean = s / (double)Lp;
    double m2 = 0.0;
    for (int l = lane; l < Lp; l += 64) {
        const double d = (double)x[l] - mean;
        m2 += d * d;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m2 += __shfl_xor(m2, o);
    if (lane == 0) {
        stat[row * 2] = (float)mean;
        stat[row * 2 + 1] = (float)(1.0 / sqrt(m2 / (double)Lp + (double)eps));
    }
}

// feats [b][t][c]: the last norm, leaky_relu and the "b f t -> b t f" rearrange
__global__ __launch_bounds__(256) void st_out_kernel(const float *p, const float *stat, const float *gamma, const float *beta, int B, int C, int L,
                                                     float slope, float *feats, const void *state, int P) {
    if (!ht_state_ok(state, SNT_MAGIC, P)) return;
    const long long n = (long long)B * L * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long bt = i / C;
        const int t = (int)(bt % L), b = (int)(bt / L);
        const size_t row = (size_t)b * C + c;
        float xh;
        feats[i] = st_leaky(st_z(p[row * L + t], stat[row * 2], stat[row * 2 + 1], gamma[c], beta[c], xh), slope);
    }
}

struct StNormBwd {
    const float *da; long long da_bs, da_cs, da_ls;   // d_a_out(b, c, l) = da[b da_bs + c da_cs + l da_ls]
    const float *p; const uint8_t *idx; const float *stat, *gamma, *beta;
    int C, Lp; float slope; int s0;
    float *dp;                   // [B][C][Lp]; may be da itself (element for element)
    float *nb;                   // [B][C][2]: the row's sum dz xhat, sum dz
    const void *state; int P; HtGuard guard;
};

__global__ __launch_bounds__(64) void st_norm_bwd_kernel(StNormBwd a) {
    if (!ht_state_ok(a.state, SNT_MAGIC, a.P) || !ht_guard_ok(a.guard)) return;
    const size_t row = blockIdx.x;
    const int b = (int)(row / a.C), c = (int)(row - (size_t)b * a.C), lane = threadIdx.x;
    const float *x = a.p + row * a.Lp;
    const float *d = a.da + (size_t)b * a.da_bs + (size_t)c * a.da_cs;
    const float mean = a.stat[row * 2], rstd = a.stat[row * 2 + 1], gamma = a.gamma[c], beta = a.beta[c];
    double g1 = 0.0, g2 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int l = lane; l < a.Lp; l += 64) {
        float xh;
        const float z = st_z(x[l], mean, rstd, gamma, beta, xh);
        const float dz = d[(size_t)l * a.da_ls] * (z > 0.0f ? 1.0f : a.slope);
        const float dxh = dz * gamma;
        g1 += (double)dz;
        g2 += (double)(dz * xh);
        s1 += (double)dxh;
        s2 += (double)(dxh * xh);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { g1 += __shfl_xor(g1, o); g2 += __shfl_xor(g2, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    const float m1 = (float)(s1 / (double)a.Lp), m2 = (float)(s2 / (double)a.Lp);
    for (int l = lane; l < a.Lp; l += 64) {
        float xh;
        const float z = st_z(x[l], mean, rstd, gamma, beta, xh);
        const float dz = d[(size_t)l * a.da_ls] * (z > 0.0f ? 1.0f : a.slope);
        const float dxh = dz * gamma;
        float v = rstd * ((dxh - m1) - xh * m2);
        if (a.s0) {
            const int sg = a.idx[row * a.Lp + l] >> 2;
            v = sg == 1 ? v : sg == 2 ? -v : 0.0f;   // sign(+-0) = 0, as torch.abs's gradient
        }
        a.dp[row * a.Lp + l] = v;
    }
    if (lane == 0) { a.nb[row * 2] = (float)g2; a.nb[row * 2 + 1] = (float)g1; }
}

// d gamma_c, d beta_c = the rows' shares in row order, into segment 0 of the partials (+0 in the others)
__global__ __launch_bounds__(128) void st_cfold_kernel(const float *nb, int B, int C, float *part, int off_g, int off_b, int nseg, int Pp,
                                                       const void *state, int P, HtGuard guard) {
    if (!ht_state_ok(state, SNT_MAGIC, P) || !ht_guard_ok(guard)) return;
    const int c = threadIdx.x;
    if (c >= C) return;
    double sg = 0.0, sb = 0.0;
    for (int b = 0; b < B; ++b) { sg += (double)nb[((size_t)b * C + c) * 2]; sb += (double)nb[((size_t)b * C + c) * 2 + 1]; }
    part[off_g + c] = (float)sg;
    part[off_b + c] = (float)sb;
    for (int z = 1; z < nseg; ++z) { part[(size_t)z * Pp + off_g + c] = 0.0f; part[(size_t)z * Pp + off_b + c] = 0.0f; }
}

struct StWgrad {
    StIn in;
    const float *dp; const uint8_t *idx;   // [B][Cout][Lp]
    int Cout, Nc, Kw, stride, Lp, L3;      // Nc = Cin Kw, L3 = 3 Lp
    long long K;                           // B L3 flat conv positions
    float *C, *Cb; long long part_stride; int seg;
    const void *state; int P; HtGuard guard;
};

template <bool S0>
__global__ __launch_bounds__(256) void st_wgrad_kernel(StWgrad g) {
    __shared__ float As[HT_KC * HT_LD], Bs[HT_KC * HT_LD];
    if (!ht_state_ok(g.state, SNT_MAGIC, g.P) || !ht_guard_ok(g.guard)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_n = (g.Nc + HT_TN - 1) / HT_TN;
    const int m0 = (int)(blockIdx.x / (unsigned)tiles_n) * HT_TM, n0 = (int)(blockIdx.x % (unsigned)tiles_n) * HT_TN;
    const long long kb = (long long)blockIdx.y * g.seg;
    const long long ke = kb + g.seg < g.K ? kb + g.seg : g.K;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    float bsum = 0.0f;
    for (long long k0 = kb; k0 < ke; k0 += HT_KC) {
#pragma unroll
        for (int i = 0; i < HT_TM * HT_KC / 256; ++i) {
            const int e = tid + 256 * i, kk = e % HT_KC, mm = e / HT_KC;
            const int m = m0 + mm;
            const long long k = k0 + kk;
            float v = 0.0f;
            if (m < g.Cout && k < ke) {
                const int b = (int)(k / g.L3), t = (int)(k - (long long)b * g.L3);
                v = st_du(g.dp, g.idx, b, g.Cout, g.Lp, m, t);
            }
            As[kk * HT_LD + mm] = v;
        }
#pragma unroll
        for (int i = 0; i < HT_TN * HT_KC / 256; ++i) {
            const int e = tid + 256 * i;
            int nn, kk;
            if (S0) { nn = e % HT_TN; kk = e / HT_TN; } else { kk = e % HT_KC; nn = e / HT_KC; }
            const int n = n0 + nn;
            const long long k = k0 + kk;
            float v = 0.0f;
            if (n < g.Nc && k < ke) {
                const int b = (int)(k / g.L3), t = (int)(k - (long long)b * g.L3);
                const int ci = n / g.Kw, tap = n - ci * g.Kw;
                v = st_in<S0, true>(g.in, b, ci, (long long)t * g.stride + tap);
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
        if (n0 == 0 && tid < HT_TM) {   // the chunk's 32 positions in order, then the chunks in order: ht_gemm_kernel<2>'s bias partial
            float c = 0.0f;
#pragma unroll
            for (int kk = 0; kk < HT_KC; ++kk) c += As[kk * HT_LD + tid];
            bsum += c;
        }
        __syncthreads();
    }
    float *C = g.C + (size_t)blockIdx.y * g.part_stride;
    const int n = n0 + wn + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.Cout || n >= g.Nc) continue;
        C[(size_t)m * g.Nc + n] = acc[r];
    }
    if (n0 == 0 && tid < HT_TM && m0 + tid < g.Cout) g.Cb[(size_t)blockIdx.y * g.part_stride + m0 + tid] = bsum;
}

struct StDgrad {
    const float *dp; const uint8_t *idx; int Cout, Lp, L3;   // the upper stage
    const float *W; int Cin, Kw, K;                          // W [Cout][Cin][Kw], K = Cout Kw
    float *out; int Lin;                                     // d_a_out of the stage below [B][Cin][Lin]
    const void *state; int P; HtGuard guard;
};

__global__ __launch_bounds__(256) void st_dgrad_kernel(StDgrad g) {
    __shared__ float As[HT_KC * HT_LD], Bs[HT_KC * HT_LD];
    if (!ht_state_ok(g.state, SNT_MAGIC, g.P) || !ht_guard_ok(g.guard)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int tiles_n = (g.Lin + HT_TN - 1) / HT_TN;
    const int m0 = (int)(blockIdx.x / (unsigned)tiles_n) * HT_TM, n0 = (int)(blockIdx.x % (unsigned)tiles_n) * HT_TN;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < g.K; k0 += HT_KC) {
#pragma unroll
        for (int i = 0; i < HT_TM * HT_KC / 256; ++i) {
            const int e = tid + 256 * i, mm = e % HT_TM, kk = e / HT_TM;
            const int m = m0 + mm, k = k0 + kk;
            float v = 0.0f;
            if (m < g.Cin && k < g.K) {
                const int co = k / g.Kw, tap = k - co * g.Kw;
                v = g.W[((size_t)co * g.Cin + m) * g.Kw + tap];
            }
            As[kk * HT_LD + mm] = v;
        }
#pragma unroll
        for (int i = 0; i < HT_TN * HT_KC / 256; ++i) {
            const int e = tid + 256 * i, nn = e % HT_TN, kk = e / HT_TN;
            const int n = n0 + nn, k = k0 + kk;
            float v = 0.0f;
            if (n < g.Lin && k < g.K) {
                const int co = k / g.Kw, tap = k - co * g.Kw, t = n - tap;
                if (t >= 0 && t < g.L3) v = st_du(g.dp, g.idx, b, g.Cout, g.Lp, co, t);
            }
            Bs[kk * HT_LD + nn] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < HT_KC; kk += 2) {
            const float a = As[(kk + (lane >> 5)) * HT_LD + wm + (lane & 31)];
            const float bb = Bs[(kk + (lane >> 5)) * HT_LD + wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int n = n0 + wn + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.Cin || n >= g.Lin) continue;
        g.out[((size_t)b * g.Cin + m) * g.Lin + n] = acc[r];
    }
}

// Gf[j] = stage 0's partials of G [NF][KS] and D [NF] in segment order
__global__ __launch_bounds__(256) void st_gfold_kernel(const float *part, int nseg, int GS, int n, float *Gf, const void *state, int P, HtGuard guard) {
    if (!ht_state_ok(state, SNT_MAGIC, P) || !ht_guard_ok(guard)) return;
    const int j = (int)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float s = part[j];
    for (int z = 1; z < nseg; ++z) s = s + part[(size_t)z * GS + j];
    Gf[j] = s;
}

struct StBankBwd {
    const float *Gf;             // G [NF][KS] then D [NF]
    const float *bank, *low, *band, *win, *nn, *wg, *wb;
    int NF, KS;
    float *part; int off[4]; int nseg, Pp;   // wav_norm1d.weight, .bias, low_hz_, band_hz_
    const void *state; int P; HtGuard guard;
};

// one workgroup: thread c' < NF the row sums of F G and F, thread c < NF / 2 the chain rule of band pair c, thread 0 the two scalars
__global__ __launch_bounds__(256) void st_bank_bwd_kernel(StBankBwd a) {
    __shared__ double fg[256], fsum[256];
    if (!ht_state_ok(a.state, SNT_MAGIC, a.P) || !ht_guard_ok(a.guard)) return;
    const int tid = threadIdx.x, half = a.KS / 2, cut = a.NF / 2;
    const float *D = a.Gf + (size_t)a.NF * a.KS;
    const double g = (double)a.wg[0], b0 = (double)a.wb[0];
    for (int c = tid; c < a.NF; c += 256) {
        double s = 0.0, f = 0.0;
        for (int k = 0; k < a.KS; ++k) {
            const double F = (double)a.bank[(size_t)c * a.KS + k];
            s += F * (double)a.Gf[(size_t)c * a.KS + k];
            f += F;
        }
        fg[c] = s; fsum[c] = f;
    }
    for (int c = tid; c < cut; c += 256) {
        const StEdges q = st_edges(a.low[c], a.band[c]);
        const float *Gc = a.Gf + (size_t)c * a.KS, *Gs = a.Gf + (size_t)(c + cut) * a.KS;
        const double Dc = b0 * (double)D[c], Ds = b0 * (double)D[c + cut];
        double dH = 0.0, dL = 0.0, Q = 0.0;
        for (int i = 0; i < half; ++i) {
            const double gc = (g * (double)Gc[i] + Dc) + (g * (double)Gc[a.KS - 1 - i] + Dc);
            const double gs = (g * (double)Gs[i] + Ds) - (g * (double)Gs[a.KS - 1 - i] + Ds);
            const double n = (double)a.nn[i], w = (double)a.win[i];
            const double fl = q.low * n, fh = q.high * n;
            const double sfl = sin(fl), cfl = cos(fl), sfh = sin(fh), cfh = cos(fh);
            dH += (w / q.bandw) * (gc * cfh + gs * sfh);
            dL -= (w / q.bandw) * (gc * cfl + gs * sfl);
            Q += (gc * (sfh - sfl) + gs * (cfl - cfh)) * w / (n * q.bandw);
        }
        const double dB = -Q / q.bandw;            // band = high - low
        const double dhigh = dH + dB;
        double dlow = dL - dB;
        const double draw = q.pass ? dhigh : 0.0;  // torch.clamp passes a gradient only inside [min, max]
        dlow += draw;
        const float lp = a.low[c], bp = a.band[c];
        const float glow = (float)(lp > 0.0f ? dlow : lp < 0.0f ? -dlow : 0.0);
        const float gband = (float)(bp > 0.0f ? draw : bp < 0.0f ? -draw : 0.0);
        a.part[a.off[2] + c] = glow;
        a.part[a.off[3] + c] = gband;
        for (int z = 1; z < a.nseg; ++z) { a.part[(size_t)z * a.Pp + a.off[2] + c] = 0.0f; a.part[(size_t)z * a.Pp + a.off[3] + c] = 0.0f; }
    }
    __syncthreads();
    if (tid == 0) {
        double dg = 0.0, db = 0.0;
        for (int c = 0; c < a.NF; ++c) { dg += fg[c]; db += (double)D[c] * fsum[c]; }
        a.part[a.off[0]] = (float)dg;
        a.part[a.off[1]] = (float)db;
        for (int z = 1; z < a.nseg; ++z) { a.part[(size_t)z * a.Pp + a.off[0]] = 0.0f; a.part[(size_t)z * a.Pp + a.off[1]] = 0.0f; }
    }
}

__global__ __launch_bounds__(256) void st_copy_kernel(const float *src, float *dst, int n, const void *state, int P) {
    const bool ok = ht_state_ok(state, SNT_MAGIC, P);
    for (int j = (int)blockIdx.x * 256 + threadIdx.x; j < n; j += (int)gridDim.x * 256) dst[j] = ok ? src[j] : 0.0f;
}

struct StBufs {
    SincTrainWsHead *head; HeadTrainWsHead *fold; float *wstat, *p[3], *stat[3], *g[3], *nb, *part, *partG, *Gf; uint8_t *idx[3];
};
StBufs st_bufs(const SincTrainWs &w, void *ws) {
    char *base = reinterpret_cast<char *>(ws);
    StBufs b{};
    b.head = reinterpret_cast<SincTrainWsHead *>(base);
    b.fold = reinterpret_cast<HeadTrainWsHead *>(base + w.off_fold);
    b.wstat = reinterpret_cast<float *>(base + w.off_wstat);
    for (int s = 0; s < 3; ++s) {
        b.p[s] = reinterpret_cast<float *>(base + w.off_p[s]);
        b.idx[s] = reinterpret_cast<uint8_t *>(base + w.off_idx[s]);
        b.stat[s] = reinterpret_cast<float *>(base + w.off_stat[s]);
        b.g[s] = reinterpret_cast<float *>(base + w.off_g[s]);
    }
    b.nb = reinterpret_cast<float *>(base + w.off_nb);
    b.part = reinterpret_cast<float *>(base + w.off_part);
    b.partG = reinterpret_cast<float *>(base + w.off_partG);
    b.Gf = reinterpret_cast<float *>(base + w.off_Gf);
    return b;
}

// tensor t of the state: the master when its stage learns, the frozen copy otherwise
const float *st_tensor(const SincTrainShape &q, const void *state, int t) {
    const float *base = reinterpret_cast<const float *>(reinterpret_cast<const char *>(state) + sizeof(HeadTrainHeader));
    return q.off_master[t] >= 0 ? base + q.off_master[t] : base + q.off_fullblock + q.off_full[t];
}
StIn st_stage_in(const SincTrainShape &q, const SincTrainGeo &geo, const StBufs &b, const void *state, const float *wav, long long S, int s) {
    StIn in{};
    in.slope = q.slope;
    in.Cin = q.Cin[s];
    in.Lin = (int)geo.Lin[s];
    if (s == 0) { in.x = wav; in.stat = b.wstat; in.bstride = S; return in; }
    in.x = b.p[s - 1]; in.stat = b.stat[s - 1];
    in.gamma = st_tensor(q, state, SNT_T_NORM + 2 * (s - 1)); in.beta = st_tensor(q, state, SNT_T_NORM + 2 * (s - 1) + 1);
    in.bstride = (long long)q.Cin[s] * geo.Lin[s];
    return in;
}
unsigned st_tiles(int M, int N) { return (unsigned)(((M + HT_TM - 1) / HT_TM) * ((N + HT_TN - 1) / HT_TN)); }
bool st_args_ok(const SincTrainShape &q, const SincTrainArgs &a, const SincTrainGeo &geo) {
    return a.wav && a.state && a.ws && a.B > 0 && geo.ok && a.seg >= HT_MIN_SEGMENT && a.seg <= HT_MAX_SEGMENT && a.seg % 32 == 0 &&
           (long long)a.B * geo.L[0] <= 0x7fffffffLL && q.first_stage >= 0 && q.first_stage <= 2;
}

}  // namespace

SincTrainShape sinc_train_shape(int n_filters, int kernel_size, int stride, int c2, int k2, int c3, int k3, float slope, float eps, int first_stage) {
    SincTrainShape q{};
    q.first_stage = first_stage; q.NF = n_filters; q.KS = kernel_size; q.stride = stride; q.slope = slope; q.eps = eps;
    const int cin[3] = {1, n_filters, c2}, cout[3] = {n_filters, c2, c3}, kw[3] = {kernel_size, k2, k3};
    for (int s = 0; s < 3; ++s) { q.Cin[s] = cin[s]; q.Cout[s] = cout[s]; q.Kw[s] = kw[s]; }
    const int cnt[SNT_TENSORS] = {1, 1, n_filters / 2, n_filters / 2, c2 * n_filters * k2, c2, c3 * c2 * k3, c3, n_filters, n_filters, c2, c2, c3, c3};
    const int stage[SNT_TENSORS] = {0, 0, 0, 0, 1, 1, 2, 2, 0, 0, 1, 1, 2, 2};
    int full = 0, off = 0;
    for (int t = 0; t < SNT_TENSORS; ++t) {
        q.cnt[t] = cnt[t]; q.stage_of[t] = stage[t];
        q.off_full[t] = full; full += cnt[t];
        if (stage[t] >= first_stage) { q.off_master[t] = off; off += cnt[t]; } else q.off_master[t] = -1;
    }
    q.P = off; q.Pp = (off + 63) / 64 * 64;
    q.Pfull = full; q.Pfullp = (full + 63) / 64 * 64;
    q.bankp = (n_filters * kernel_size + 63) / 64 * 64;
    q.halfp = (kernel_size / 2 + 63) / 64 * 64;
    q.off_bank = 4 * q.Pp;
    q.off_fullblock = q.off_bank + q.bankp;
    q.off_win = q.off_fullblock + q.Pfullp;
    q.off_n = q.off_win + q.halfp;
    return q;
}

size_t sinc_train_state_bytes(const SincTrainShape &q) { return sizeof(HeadTrainHeader) + (size_t)(q.off_n + q.halfp) * sizeof(float); }

SincTrainGeo sinc_train_geo(const SincTrainShape &q, long long S) {
    SincTrainGeo g{};
    long long L = S;
    g.ok = S > 0;
    for (int s = 0; s < 3; ++s) {
        const int st = s == 0 ? q.stride : 1;
        g.Lin[s] = L;
        g.L[s] = L >= q.Kw[s] ? (L - q.Kw[s]) / st + 1 : 0;
        g.Lp[s] = g.L[s] / 3;
        if (g.Lp[s] <= 0) g.ok = false;
        L = g.Lp[s];
    }
    return g;
}

SincTrainWs sinc_train_ws(const SincTrainShape &q, const SincTrainGeo &geo, int B, int seg) {
    SincTrainWs w{};
    const size_t f = sizeof(float);
    const long long K = (long long)B * 3 * geo.Lp[q.first_stage];
    w.nseg = (int)((K + seg - 1) / seg);
    w.GS = (q.NF * q.KS + q.NF + 63) / 64 * 64;
    size_t off = sizeof(SincTrainWsHead);
    w.off_fold = off; off += sizeof(HeadTrainWsHead);
    w.off_wstat = off; off = ht_align(off + (size_t)B * 4 * f);
    int cmax = 0;
    for (int s = 0; s < 3; ++s) {
        const size_t n = (size_t)B * q.Cout[s] * (size_t)geo.Lp[s];
        w.off_p[s] = off; off = ht_align(off + n * f);
        w.off_idx[s] = off; off = ht_align(off + n);
        w.off_stat[s] = off; off = ht_align(off + (size_t)B * q.Cout[s] * 2 * f);
        w.off_g[s] = off; off = ht_align(off + (s >= q.first_stage ? n * f : 0));
        cmax = q.Cout[s] > cmax ? q.Cout[s] : cmax;
    }
    w.off_nb = off; off = ht_align(off + (size_t)B * cmax * 2 * f);
    w.off_part = off; off = ht_align(off + (size_t)w.nseg * q.Pp * f);
    w.off_partG = off; off = ht_align(off + (q.first_stage == 0 ? (size_t)w.nseg * w.GS * f : 0));
    w.off_Gf = off; off = ht_align(off + (q.first_stage == 0 ? (size_t)w.GS * f : 0));
    w.total = off;
    return w;
}

#define ST_LAUNCHED() do { e = hipGetLastError(); if (e != hipSuccess) return e; } while (0)

hipError_t launch_sinc_train_forward(const SincTrainShape &q, const SincTrainArgs &a, hipStream_t s) {
    const SincTrainGeo geo = sinc_train_geo(q, a.S);
    if (!st_args_ok(q, a, geo) || !a.feats) return hipErrorInvalidValue;
    const SincTrainWs w = sinc_train_ws(q, geo, a.B, a.seg);
    const StBufs b = st_bufs(w, a.ws);
    float *base = reinterpret_cast<float *>(reinterpret_cast<char *>(a.state) + sizeof(HeadTrainHeader));
    hipError_t e;
    // a frozen stage 0 runs the same bank when the state has the band edges: feats do not depend on first_stage
    e = launch_sinc_train_bank(q, a.state, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(st_wav_stats_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a.wav, a.B, a.S, st_tensor(q, a.state, SNT_T_WAV),
                       st_tensor(q, a.state, SNT_T_WAV + 1), q.eps, b.wstat, b.head, (const void *)a.state, q.P);
    ST_LAUNCHED();
    for (int st = 0; st < 3; ++st) {
        StConv c{};
        c.in = st_stage_in(q, geo, b, a.state, a.wav, a.S, st);
        c.W = st == 0 ? base + q.off_bank : st_tensor(q, a.state, SNT_T_CONV + 2 * (st - 1));
        c.bias = st == 0 ? nullptr : st_tensor(q, a.state, SNT_T_CONV + 2 * (st - 1) + 1);
        c.Cout = q.Cout[st]; c.K = q.Cin[st] * q.Kw[st]; c.Kw = q.Kw[st]; c.stride = st == 0 ? q.stride : 1; c.Lp = (int)geo.Lp[st];
        c.p = b.p[st]; c.idx = b.idx[st]; c.state = a.state; c.P = q.P;
        const dim3 grid(st_tiles(c.Cout, c.Lp), (unsigned)a.B);
        if (st == 0) hipLaunchKernelGGL(st_conv_kernel<true>, grid, dim3(256), 0, s, c);
        else hipLaunchKernelGGL(st_conv_kernel<false>, grid, dim3(256), 0, s, c);
        ST_LAUNCHED();
        hipLaunchKernelGGL(st_stats_kernel, dim3((unsigned)(a.B * q.Cout[st])), dim3(64), 0, s, (const float *)b.p[st], (int)geo.Lp[st], q.eps,
                           b.stat[st], (const void *)a.state, q.P);
        ST_LAUNCHED();
    }
    const long long n = (long long)a.B * geo.Lp[2] * q.Cout[2];
    hipLaunchKernelGGL(st_out_kernel, dim3((unsigned)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536)), dim3(256), 0, s, (const float *)b.p[2],
                       (const float *)b.stat[2], st_tensor(q, a.state, SNT_T_NORM + 4), st_tensor(q, a.state, SNT_T_NORM + 5), a.B, q.Cout[2],
                       (int)geo.Lp[2], q.slope, a.feats, (const void *)a.state, q.P);
    ST_LAUNCHED();
    return hipSuccess;
}

hipError_t launch_sinc_train_backward(const SincTrainShape &q, const SincTrainArgs &a, hipStream_t s) {
    const SincTrainGeo geo = sinc_train_geo(q, a.S);
    if (!st_args_ok(q, a, geo) || !a.dfeats) return hipErrorInvalidValue;
    const SincTrainWs w = sinc_train_ws(q, geo, a.B, a.seg);
    if (w.nseg > 65535) return hipErrorInvalidValue;
    const StBufs b = st_bufs(w, a.ws);
    float *base = reinterpret_cast<float *>(reinterpret_cast<char *>(a.state) + sizeof(HeadTrainHeader));
    const HtGuard guard{reinterpret_cast<const int *>(b.head), {SNT_WS_MAGIC ^ (int)(a.S >> 32), a.B, (int)a.S}};
    hipError_t e;
    for (int st = 2; st >= q.first_stage; --st) {
        const int C = q.Cout[st], Lp = (int)geo.Lp[st];
        const int tg = SNT_T_NORM + 2 * st;
        StNormBwd nb{};
        if (st == 2) { nb.da = a.dfeats; nb.da_bs = (long long)Lp * C; nb.da_cs = 1; nb.da_ls = C; }
        else { nb.da = b.g[st]; nb.da_bs = (long long)C * Lp; nb.da_cs = Lp; nb.da_ls = 1; }
        nb.p = b.p[st]; nb.idx = b.idx[st]; nb.stat = b.stat[st]; nb.gamma = st_tensor(q, a.state, tg); nb.beta = st_tensor(q, a.state, tg + 1);
        nb.C = C; nb.Lp = Lp; nb.slope = q.slope; nb.s0 = st == 0; nb.dp = b.g[st]; nb.nb = b.nb;
        nb.state = a.state; nb.P = q.P; nb.guard = guard;
        hipLaunchKernelGGL(st_norm_bwd_kernel, dim3((unsigned)(a.B * C)), dim3(64), 0, s, nb);
        ST_LAUNCHED();
        hipLaunchKernelGGL(st_cfold_kernel, dim3(1), dim3(128), 0, s, (const float *)b.nb, a.B, C, b.part, q.off_master[tg], q.off_master[tg + 1],
                           w.nseg, q.Pp, (const void *)a.state, q.P, guard);
        ST_LAUNCHED();
        StWgrad g{};
        g.in = st_stage_in(q, geo, b, a.state, a.wav, a.S, st);
        g.dp = b.g[st]; g.idx = b.idx[st]; g.Cout = C; g.Nc = q.Cin[st] * q.Kw[st]; g.Kw = q.Kw[st]; g.stride = st == 0 ? q.stride : 1;
        g.Lp = Lp; g.L3 = 3 * Lp; g.K = (long long)a.B * g.L3; g.seg = a.seg;
        g.state = a.state; g.P = q.P; g.guard = guard;
        const dim3 grid(st_tiles(C, g.Nc), (unsigned)w.nseg);
        if (st == 0) {
            g.C = b.partG; g.Cb = b.partG + (size_t)q.NF * q.KS; g.part_stride = w.GS;
            hipLaunchKernelGGL(st_wgrad_kernel<true>, grid, dim3(256), 0, s, g);
        } else {
            const int tc = SNT_T_CONV + 2 * (st - 1);
            g.C = b.part + q.off_master[tc]; g.Cb = b.part + q.off_master[tc + 1]; g.part_stride = q.Pp;
            hipLaunchKernelGGL(st_wgrad_kernel<false>, grid, dim3(256), 0, s, g);
        }
        ST_LAUNCHED();
        if (st > q.first_stage) {
            StDgrad d{};
            d.dp = b.g[st]; d.idx = b.idx[st]; d.Cout = C; d.Lp = Lp; d.L3 = 3 * Lp;
            d.W = st_tensor(q, a.state, SNT_T_CONV + 2 * (st - 1)); d.Cin = q.Cin[st]; d.Kw = q.Kw[st]; d.K = C * q.Kw[st];
            d.out = b.g[st - 1]; d.Lin = (int)geo.Lin[st];
            d.state = a.state; d.P = q.P; d.guard = guard;
            hipLaunchKernelGGL(st_dgrad_kernel, dim3(st_tiles(d.Cin, d.Lin), (unsigned)a.B), dim3(256), 0, s, d);
            ST_LAUNCHED();
        }
    }
    if (q.first_stage == 0) {
        const int n = q.NF * q.KS + q.NF;
        hipLaunchKernelGGL(st_gfold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)b.partG, w.nseg, w.GS, n, b.Gf,
                           (const void *)a.state, q.P, guard);
        ST_LAUNCHED();
        StBankBwd k{};
        k.Gf = b.Gf; k.bank = base + q.off_bank; k.low = st_tensor(q, a.state, SNT_T_LOW); k.band = st_tensor(q, a.state, SNT_T_BAND);
        k.win = base + q.off_win; k.nn = base + q.off_n; k.wg = st_tensor(q, a.state, SNT_T_WAV); k.wb = st_tensor(q, a.state, SNT_T_WAV + 1);
        k.NF = q.NF; k.KS = q.KS; k.part = b.part; k.nseg = w.nseg; k.Pp = q.Pp;
        for (int t = 0; t < 4; ++t) k.off[t] = q.off_master[t];
        k.state = a.state; k.P = q.P; k.guard = guard;
        hipLaunchKernelGGL(st_bank_bwd_kernel, dim3(1), dim3(256), 0, s, k);
        ST_LAUNCHED();
    }
    hipLaunchKernelGGL(ht_fold_kernel, dim3((unsigned)((q.P + 255) / 256)), dim3(256), 0, s, a.state, SNT_MAGIC, q.P, q.Pp, (const float *)b.part,
                       w.nseg, (const double *)nullptr, 0, 0, (const int *)nullptr, a.B, (int)geo.Lp[2], b.fold, guard);
    ST_LAUNCHED();
    return hipSuccess;
}
#undef ST_LAUNCHED

// the bank from the masters as they stand (uvad_sincnet_train_commit: what is served matches the committed band edges)
hipError_t launch_sinc_train_bank(const SincTrainShape &q, void *state, hipStream_t s) {
    if (!state) return hipErrorInvalidValue;
    float *base = reinterpret_cast<float *>(reinterpret_cast<char *>(state) + sizeof(HeadTrainHeader));
    StBank k{};
    k.low = st_tensor(q, state, SNT_T_LOW); k.band = st_tensor(q, state, SNT_T_BAND); k.win = base + q.off_win; k.nn = base + q.off_n;
    k.bank = base + q.off_bank; k.NF = q.NF; k.KS = q.KS; k.state = state; k.P = q.P;
    hipLaunchKernelGGL(st_bank_kernel, dim3((unsigned)(((q.NF / 2) * (q.KS / 2) + 255) / 256)), dim3(256), 0, s, k);
    return hipGetLastError();
}

// which = UVAD_SINCNET_TRAIN_FILTERS of uvad_sincnet_train_read: the bank of the last forward call (every other block: launch_train_read)
hipError_t launch_sinc_train_read_bank(const SincTrainShape &q, const void *state, float *out, hipStream_t s) {
    if (!state || !out) return hipErrorInvalidValue;
    const float *bank = reinterpret_cast<const float *>(reinterpret_cast<const char *>(state) + sizeof(HeadTrainHeader)) + q.off_bank;
    const int n = q.NF * q.KS;
    hipLaunchKernelGGL(st_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bank, out, n, state, q.P);
    return hipGetLastError();
}

}  // namespace uvad
