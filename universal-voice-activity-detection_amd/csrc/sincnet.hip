// sincnet.hip -- SincNet front end of PyanNet (reference: src/models/blocks/sincnet.py:33-103, called from
// PyanNet.forward, src/models/segmentation/PyanNet.py:177).  waveform (B, S) -> features (B, frames, 60):
//
//   wav_norm1d (InstanceNorm1d(1))                                   -> wav_stats_kernel   (scale, shift per b; int16: wav_stats_i16_kernel)
//   sinc filter bank conv (80 x 251, stride 10), |.|, MaxPool1d(3)   -> conv_pool_kernel<3, true>
//   InstanceNorm1d(80) + leaky_relu                                  -> norm_finalize_kernel (scale, shift per (b, c)),
//                                                                       applied when the NEXT conv stages its input
//   Conv1d(80, 60, 5), MaxPool1d(3)                                  -> conv_pool_kernel<2, false>
//   InstanceNorm1d(60) + leaky_relu
//   Conv1d(60, 60, 5), MaxPool1d(3)                                  -> conv_pool_kernel<2, false>
//   InstanceNorm1d(60) + leaky_relu, "b f t -> b t f"                -> sinc_out_kernel
//
// The convolutions are implicit GEMMs on the f32 matrix cores (v_mfma_f32_32x32x2_f32, exact f32 products and
// a k-ordered accumulation): a workgroup of 3 waves owns 96 consecutive conv positions (= 32 pooled outputs)
// x all output channels; the whole transposed filter matrix ([K][N]: one conflict-free ds_read_b32 per lane
// feeds the B operand) stays in LDS across the tiles a workgroup walks; the input window of the NEXT tile is
// fetched into registers while the matrix cores work on the current one and is written to LDS with the
// previous layer's normalisation + leaky_relu folded in; the epilogue does
// bias, |.|, the 3:1 max pool and the per-tile (sum, M2) statistics the instance norm of the next stage
// needs -- written as per-tile partials and reduced in tile order, so results do not depend on scheduling.
#include "uvad_internal.h"

#include <type_traits>

namespace uvad {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// Sum over each 32-lane half of the wave, returned in every lane of the half (DPP adds inside the 16-lane rows,
// row_bcast:15 into the odd rows, then the totals sit in lanes 31 and 63).  Inactive half-waves read as zero.
#define UVAD_SN_DPP_ADD(V, CTRL, ROW_MASK) \
    V += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, V), CTRL, ROW_MASK, 0xF, true))
__device__ __forceinline__ float half_sum(float v, bool upper) {
    UVAD_SN_DPP_ADD(v, 0xB1, 0xF);    // quad_perm [1,0,3,2]
    UVAD_SN_DPP_ADD(v, 0x4E, 0xF);    // quad_perm [2,3,0,1]
    UVAD_SN_DPP_ADD(v, 0x141, 0xF);   // row_half_mirror
    UVAD_SN_DPP_ADD(v, 0x140, 0xF);   // row_mirror: every lane holds its row total
    UVAD_SN_DPP_ADD(v, 0x142, 0xA);   // row_bcast:15 into rows 1 and 3
    const float lo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 31));
    const float hi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
    return upper ? hi : lo;
}

constexpr int YS = 97;        // LDS row stride of the conv-output staging tile

// LENS (uvad_sincnet_lens): row b's statistics over its first row_n[b] samples (0: scale = shift = 0, nothing read).  The sums take the
// order of the 16-byte-aligned path even where the row start is not aligned (rows of a padded batch), so every row reaches the bits of a
// dense call on that row alone in its own (aligned) buffer for any f32 samples, not only for sums that are exact.
template <bool LENS>
__global__ __launch_bounds__(1024) void wav_stats_kernel(const float *wav, long long S, long long row_stride, const float *gamma,
                                                         const float *beta, float eps, float *scale, float *shift, SincRowTArg<LENS> row_n) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *x = wav + (size_t)b * row_stride;
    if constexpr (LENS) {
        S = row_n[b];
        if (S <= 0) {
            if (tid == 0) { scale[b] = 0.f; shift[b] = 0.f; }
            return;
        }
    }
    double s = 0.0, ss = 0.0;
    long long i0 = 0;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    if (vec || LENS) {   // 16-byte loads, 1024 threads: the whole row is in flight at once
        const long long n4 = S >> 2;
        for (long long i = tid; i < n4; i += 1024) {
            float4 v;
            if (!LENS || vec) v = reinterpret_cast<const float4 *>(x)[i];
            else v = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
            s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
            ss += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
        }
        i0 = n4 << 2;
    }
    for (long long i = i0 + tid; i < S; i += 1024) {
        const double v = x[i];
        s += v;
        ss += v * v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); }
    __shared__ double red[2][16];
    if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = ss; }
    __syncthreads();
    if (tid == 0) {
        s = 0.0; ss = 0.0;
        for (int w = 0; w < 16; ++w) { s += red[0][w]; ss += red[1][w]; }
        const double mean = s / (double)S;
        double var = ss / (double)S - mean * mean;
        if (var < 0.0) var = 0.0;
        const double sc = (double)gamma[0] / sqrt(var + (double)eps);
        scale[b] = (float)sc;
        shift[b] = (float)((double)beta[0] - mean * sc);
    }
}

// The same statistics of int16 samples read as q / 32768 (wav ingest, uvad_sincnet_i16 / uvad_forward_wav_i16): the raw integers are summed
// exactly in int64 and scaled once.  The f32 kernel's double sums of q / 32768 are exact as well, in any order, while S < 2^23 (524 s per
// row): every term of the sum is a multiple of 2^-15 and every square a multiple of 2^-30, each of magnitude <= 1, so a 53-bit significand
// holds every partial sum.  Both kernels therefore reach the same (s, ss) and, through the same closing arithmetic, (scale, shift) that are
// bit-identical to the f32 call on q.float() / 32768 for S < 2^23; longer rows get the exact statistics here.
// LENS: over the first row_n[b] samples, as wav_stats_kernel (the integer sums are exact in any order)
template <bool LENS>
__global__ __launch_bounds__(1024) void wav_stats_i16_kernel(const int16_t *wav, long long S, long long row_stride, const float *gamma,
                                                             const float *beta, float eps, float *scale, float *shift, SincRowTArg<LENS> row_n) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int16_t *x = wav + (size_t)b * row_stride;
    if constexpr (LENS) {
        S = row_n[b];
        if (S <= 0) {
            if (tid == 0) { scale[b] = 0.f; shift[b] = 0.f; }
            return;
        }
    }
    long long s = 0, ss = 0;
    long long i0 = 0;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {   // 16-byte loads (8 samples)
        const long long n8 = S >> 3;
        for (long long i = tid; i < n8; i += 1024) {
            const int4 v = reinterpret_cast<const int4 *>(x)[i];
            const int w[4] = {v.x, v.y, v.z, v.w};
            int cs = 0;
            unsigned long long css = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int lo = (int)(int16_t)(w[k] & 0xffff), hi = w[k] >> 16;   // little endian: sample 2k in the low half
                cs += lo + hi;
                css += (unsigned)(lo * lo) + (unsigned)(hi * hi);               // <= 2^31 per pair
            }
            s += cs;
            ss += (long long)css;
        }
        i0 = n8 << 3;
    }
    for (long long i = i0 + tid; i < S; i += 1024) {
        const int v = x[i];
        s += v;
        ss += (long long)(v * v);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); }
    __shared__ long long red[2][16];
    if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = ss; }
    __syncthreads();
    if (tid == 0) {
        s = 0; ss = 0;
        for (int w = 0; w < 16; ++w) { s += red[0][w]; ss += red[1][w]; }
        const double sd = (double)s * 0x1p-15, ssd = (double)ss * 0x1p-30;   // exact while |s| < 2^53, ss < 2^53 (S < 2^23)
        const double mean = sd / (double)S;
        double var = ssd / (double)S - mean * mean;
        if (var < 0.0) var = 0.0;
        const double sc = (double)gamma[0] / sqrt(var + (double)eps);
        scale[b] = (float)sc;
        shift[b] = (float)((double)beta[0] - mean * sc);
    }
}

// a waveform sample as the stages stage it: f32 as given, int16 scaled by 2^-15 (exact: the f32 value of q / 32768)
__device__ __forceinline__ float wav_sample(float v) { return v; }
__device__ __forceinline__ float wav_sample(int16_t v) { return (float)v * 0x1p-15f; }

// I16: the single-channel stage reads the waveform as int16 (a.in_i16), converted in the prefetch with wav_sample
// LENS (uvad_sincnet_lens): the workgroups share the valid (row, tile) pairs of the rows' own lengths (SincRowCursor); the window and the
// pooled outputs are bounded by the row's Lin / Lpool (a.Lin / a.Lpool stay the padded strides): each tile is a dense call's on that row.
template <int NT, bool CIN1, int EPT, int WAVES, bool I16 = false, bool LENS = false>
__global__ __launch_bounds__(WAVES * 64) void conv_pool_kernel(SincArgsT<LENS, SincConvArgs> a) {
    static_assert(CIN1 || !I16, "int16 input is the waveform: single-channel stage only");
    using Tin = typename std::conditional<I16, int16_t, float>::type;
    constexpr int NW = NT * 32;
    constexpr int NTHR = WAVES * 64;
    constexpr int CTW = WAVES * 32;            // conv positions computed per tile (one 32-row MFMA block per wave)
    constexpr int TA = CTW / 3 * 3;            // positions the tile advances by (pool windows never straddle tiles)
    constexpr int PT = TA / 3;                 // pooled outputs per tile
    constexpr int PHASES = (WAVES + 2) / 3;    // the epilogue runs in groups of three waves = 96 positions = 32 pooled
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // (scale, shift) of the current utterance's input norm: a separate LDS object, so the compiler knows the window
    // stores below cannot alias it (with one array every store waited for the previous (scale, shift) read)
    __shared__ float2 nrm[96];
    float *wt = smem;                                  // [Kp][NW]: W^T, zero padded
    float *xy = smem + (size_t)a.Kp * NW;              // input window [Cin][XW] (+ zero pad, + 1 dump slot) / conv-output tile [NW][YS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kk = lane >> 5;
    const int XW = (CTW - 1) * a.stride + a.Kw;
    const int nelem = a.Cin * XW;                      // real elements of the window
    const int npad = 8;                                // the Kp - Ktot <= 7 zero-weight padded k read taps >= Kw: <= 7 elements past the window
    const int dump = nelem + npad;                     // where the staging stores of threads past the window go

    // Persistent workgroups (one per CU: the filter matrix takes most of the LDS): workgroup w owns the contiguous
    // range [g_begin, g_end) of the B*ntiles (utterance, tile) pairs, so the filter matrix is staged once per launch.
    long long total;
    if constexpr (LENS) total = a.rows.prefix[a.B]; else total = (long long)a.B * a.ntiles;
    const long long per = (total + gridDim.x - 1) / gridDim.x;
    const long long g_begin = per * blockIdx.x;
    const long long g_end = g_begin + per < total ? g_begin + per : total;
    if (g_begin >= g_end) return;

    {   // filter matrix -> LDS (Kp*NW is a multiple of 128 floats), 8 independent 16-byte loads in flight per thread
        const float4 *src = reinterpret_cast<const float4 *>(a.Wt2);
        float4 *dst = reinterpret_cast<float4 *>(wt);
        const int n4 = a.Kp * NW / 4;
        for (int i0 = 0; i0 < n4; i0 += NTHR * 8) {
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { const int i = i0 + j * NTHR + tid; v[j] = src[i < n4 ? i : 0]; }
#pragma unroll
            for (int j = 0; j < 8; ++j) { const int i = i0 + j * NTHR + tid; if (i < n4) dst[i] = v[j]; }
        }
    }

    // Window element e of this thread is linear index idx = tid + NTHR*e of [Cin][XW] -> (ci, x), walked incrementally.
    const int ci0 = tid / XW, xs0 = tid - ci0 * XW;
    const int qstep = NTHR / XW, rstep = NTHR - qstep * XW;
    float pre[EPT];
    const Tin *in_base;
    if constexpr (I16) in_base = a.in_i16; else in_base = a.in;
#define UVAD_SN_PREFETCH_AT(b_, tile_, lin_)                                               \
    {   /* 32-bit element offsets from the utterance's (wave-uniform) base: one address VGPR per load */ \
        const Tin *inb_ = in_base + (size_t)(b_) * a.in_bstride;                           \
        const int x0_ = (tile_) * TA * a.stride;                                           \
        int x_ = xs0;                                                                      \
        unsigned off_ = (unsigned)ci0 * (unsigned)a.Lin + (unsigned)(x0_ + xs0);           \
        _Pragma("unroll") for (int e = 0; e < EPT; ++e) {                                  \
            const bool ok_ = tid + NTHR * e < nelem && x0_ + x_ < (lin_);                  \
            pre[e] = wav_sample(inb_[ok_ ? off_ : 0u]);                                    \
            x_ += rstep; off_ += (unsigned)qstep * (unsigned)a.Lin + (unsigned)rstep;      \
            if (x_ >= XW) { x_ -= XW; off_ += (unsigned)(a.Lin - XW); }                    \
        }                                                                                  \
    }
#define UVAD_SN_PREFETCH(g_)                                                               \
    {                                                                                      \
        const int pb_ = (int)((g_) / a.ntiles), pt_ = (int)((g_) - (long long)pb_ * a.ntiles); \
        UVAD_SN_PREFETCH_AT(pb_, pt_, a.Lin)                                            \
    }
    SincRowCursor cur{}, nxt{};   // LENS: the pair g and the one after it
    if constexpr (LENS) {
        cur = sinc_cursor_seek(a.rows, a.B, g_begin);
        UVAD_SN_PREFETCH_AT(cur.b, cur.tile, cur.lin)
    } else {
        UVAD_SN_PREFETCH(g_begin)
    }

    int cur_b = -1;
    for (long long g = g_begin; g < g_end; ++g) {
        int b, tile, lin, lpool;
        if constexpr (LENS) {
            b = cur.b; tile = cur.tile; lin = cur.lin; lpool = cur.lpool;
            nxt = cur;
            if (g + 1 < g_end) sinc_cursor_next(a.rows, g + 1, nxt);
        } else {
            b = (int)(g / a.ntiles); tile = (int)(g - (long long)b * a.ntiles); lin = a.Lin; lpool = a.Lpool;
        }
        __syncthreads();   // filter matrix staged / previous tile's pooled reads of xy are complete
        if (b != cur_b) {  // (scale, shift) of this utterance's input norm
            cur_b = b;
            if (tid < a.Cin) nrm[tid] = make_float2(a.in_scale[(size_t)b * a.Cin + tid], a.in_shift[(size_t)b * a.Cin + tid]);
            __syncthreads();
        }
        {   // registers -> LDS with the previous stage's instance norm (+ leaky_relu) folded in; branch-free: threads
            // past the window store into a dump slot
            const int x0 = tile * TA * a.stride;
            int ci = ci0, x = xs0;
#pragma unroll
            for (int e0 = 0; e0 < EPT; e0 += 8) {   // eight (scale, shift) reads in flight, then eight stores
                float2 ns[8];
                bool in[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    ns[j] = nrm[ci < a.Cin ? ci : 0];
                    in[j] = x0 + x < lin;
                    ci += qstep; x += rstep;
                    if (x >= XW) { x -= XW; ++ci; }
                }
                __builtin_amdgcn_sched_barrier(0);   // keep the eight reads together (the scheduler pairs them otherwise)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int idx = tid + NTHR * (e0 + j);
                    float v = __builtin_fmaf(pre[e0 + j], ns[j].x, ns[j].y);
                    if (a.in_lrelu) v = v >= 0.f ? v : v * a.slope;
                    xy[idx < nelem ? idx : dump] = in[j] ? v : 0.f;
                }
            }
            for (int i = tid; i < npad; i += NTHR) xy[nelem + i] = 0.f;   // what the zero-weight padded K steps read
        }
        __syncthreads();
        // the next tile's window is fetched now and lands while the matrix cores work on this one
        if (g + 1 < g_end) {
            if constexpr (LENS) UVAD_SN_PREFETCH_AT(nxt.b, nxt.tile, nxt.lin) else UVAD_SN_PREFETCH(g + 1)
        }

        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

        // K loop, software pipelined over four register sets: the operands of step ks+2 are read from LDS
        // before the MFMAs of step ks are issued (sched_group_barrier pins that order), i.e. every ds_read has
        // 2*NT MFMAs (256 / 384 cycles) to land.  Kp is a multiple of 8 => ksteps is a multiple of 4.
        // K order: single-channel stage k = tap; multi-channel stages k = tap*Cin + channel (channel-minor, Cin even), so
        // the two lane halves (k, k+1) are two channels at one tap and the walk through the window is wave-uniform:
        // soff is scalar arithmetic, no per-lane wrap logic between the MFMAs (that cost 25 % of the K loop).
        const float *bp = wt + (size_t)kk * NW + li;
        const int abase = (wave * 32 + li) * a.stride + (CIN1 ? kk : kk * XW);
        int soff = 0, cpair = 0;
        const int chalf = a.Cin >> 1;
        const int ksteps = a.Kp >> 1;
        float a0, a1, a2, a3, b0[NT], b1[NT], b2[NT], b3[NT];
#define UVAD_SN_LOAD(AV, BV, ks_)                                                          \
    {                                                                                      \
        AV = xy[abase + soff];                                                             \
        _Pragma("unroll") for (int t = 0; t < NT; ++t) BV[t] = bp[(size_t)(ks_) * (NW * 2) + t * 32]; \
        if (CIN1) {                                                                        \
            soff += 2;                                                                     \
        } else {                                                                           \
            soff += 2 * XW;                                                                \
            if (++cpair == chalf) { cpair = 0; soff += 1 - a.Cin * XW; }                   \
        }                                                                                  \
    }
#define UVAD_SN_MFMA(AV, BV) \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(AV, BV[t], acc[t], 0, 0, 0);
#define UVAD_SN_GROUPS()                                                 \
    __builtin_amdgcn_sched_group_barrier(0x100, NT + 1, 0); /* DS reads */ \
    __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);     /* MFMAs    */
        UVAD_SN_LOAD(a0, b0, 0)
        UVAD_SN_LOAD(a1, b1, 1)
        int ks = 0;
        for (; ks + 4 < ksteps; ks += 4) {
            UVAD_SN_LOAD(a2, b2, ks + 2)
            UVAD_SN_MFMA(a0, b0)
            UVAD_SN_LOAD(a3, b3, ks + 3)
            UVAD_SN_MFMA(a1, b1)
            UVAD_SN_LOAD(a0, b0, ks + 4)
            UVAD_SN_MFMA(a2, b2)
            UVAD_SN_LOAD(a1, b1, ks + 5)
            UVAD_SN_MFMA(a3, b3)
            UVAD_SN_GROUPS() UVAD_SN_GROUPS() UVAD_SN_GROUPS() UVAD_SN_GROUPS()
        }
        UVAD_SN_LOAD(a2, b2, ks + 2)
        UVAD_SN_MFMA(a0, b0)
        UVAD_SN_LOAD(a3, b3, ks + 3)
        UVAD_SN_MFMA(a1, b1)
        UVAD_SN_MFMA(a2, b2)
        UVAD_SN_MFMA(a3, b3)
#undef UVAD_SN_GROUPS
#undef UVAD_SN_LOAD
#undef UVAD_SN_MFMA
        __syncthreads();   // all A reads of the input window are done: the region becomes the output tile

        // Epilogue in groups of three waves (96 positions = 32 pooled outputs, the size of the LDS output tile): bias,
        // |.|, accumulators -> LDS; 3:1 max pool; coalesced store; and the group's (sum, M2 about its own mean) per
        // channel -- combined in order by norm_finalize_kernel (Chan's update), which keeps the variance accurate when
        // it is small against the mean.  Each 32-lane half owns one channel per pass (DPP half-wave sums).
#pragma unroll
        for (int ph = 0; ph < PHASES; ++ph) {
            if (PHASES > 1 && ph > 0) __syncthreads();   // the previous group's pooled reads are complete
            if (wave / 3 == ph) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int n = t * 32 + li;
                    const float bias = a.bias[n];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
                        float v = acc[t][r] + bias;
                        if (a.do_abs) v = __builtin_fabsf(v);
                        xy[(size_t)n * YS + (wave % 3) * 32 + row] = v;
                    }
                }
            }
            __syncthreads();
            const int cap = ph == PHASES - 1 ? PT - 32 * (PHASES - 1) : 32;
            const int p0 = tile * PT + 32 * ph;
            int nt = lpool - p0 < cap ? lpool - p0 : cap;
            if (nt < 0) nt = 0;
            const float inv_nt = nt > 0 ? 1.0f / (float)nt : 0.f;
            constexpr int PASSES = (NW + 2 * WAVES - 1) / (2 * WAVES);
#pragma unroll 4
            for (int j = 0; j < PASSES; ++j) {
                const int n = j * 2 * WAVES + wave * 2 + kk, p = li;
                const int nc = n < NW ? n : NW - 1;
                const float *y = xy + (size_t)nc * YS + 3 * p;
                const float m = __builtin_fmaxf(__builtin_fmaxf(y[0], y[1]), y[2]);
                const bool valid = n < a.Cout && p < nt;
                if (valid) a.out[((size_t)b * a.Cout + n) * a.Lpool + p0 + p] = m;
                const float s = half_sum(valid ? m : 0.f, kk != 0);
                const float d = valid ? m - s * inv_nt : 0.f;
                const float m2 = half_sum(d * d, kk != 0);
                if (p == 0 && n < NW) {
                    float *pp = a.partials + (((size_t)b * a.ntiles + tile) * PHASES + ph) * (NW * 2) + n * 2;
                    pp[0] = s;
                    pp[1] = m2;
                }
            }
        }
        if constexpr (LENS) cur = nxt;
    }
#undef UVAD_SN_PREFETCH
#undef UVAD_SN_PREFETCH_AT
}

// per-tile (sum, M2) partials, combined in tile order -> per (b, c) affine of the instance norm:
//   y = (x - mean) / sqrt(var + eps) * gamma + beta = x * scale + shift      (biased variance, torch InstanceNorm1d)
// LENS: row b walks its own prefix[b + 1] - prefix[b] tiles over L_b = lpool[b] positions (`ntiles` stays the padded row
// stride of the partials): the groups and order of a dense call of that length.  L_b = 0: scale = shift = 0.
template <bool LENS>
__global__ __launch_bounds__(128) void norm_finalize_kernel(const float *partials, int ntiles, int pt, int phases, int NW, int C, int L,
                                                            const float *gamma, const float *beta, float eps, float *scale, float *shift,
                                                            SincRowsArg<LENS> rows) {
    const int b = blockIdx.x, n = threadIdx.x;
    if (n >= C) return;
    int nrow = ntiles;
    if constexpr (LENS) {
        nrow = rows.prefix[b + 1] - rows.prefix[b];
        L = rows.lpool[b];
        if (L <= 0) {
            scale[(size_t)b * C + n] = 0.f;
            shift[(size_t)b * C + n] = 0.f;
            return;
        }
    }
    double mean = 0.0, M2 = 0.0, cnt = 0.0;
    for (int t = 0; t < nrow; ++t)
        for (int ph = 0; ph < phases; ++ph) {   // the statistics groups of conv_pool_kernel, in position order
            const int start = t * pt + 32 * ph, cap = ph == phases - 1 ? pt - 32 * (phases - 1) : 32;
            const int ni = L - start < cap ? L - start : cap;
            if (ni <= 0) continue;
            const float *pp = partials + (((size_t)b * ntiles + t) * phases + ph) * (NW * 2) + n * 2;
            const double nt = (double)ni;
            const double mt = (double)pp[0] / nt, delta = mt - mean, tot = cnt + nt;
            M2 += (double)pp[1] + delta * delta * cnt * nt / tot;
            mean += delta * nt / tot;
            cnt = tot;
        }
    const double var = M2 / (double)L;
    const double sc = (double)gamma[n] / sqrt(var + (double)eps);
    scale[(size_t)b * C + n] = (float)sc;
    shift[(size_t)b * C + n] = (float)((double)beta[n] - mean * sc);
}

// last norm + leaky_relu and the "batch feature frames -> batch frames feature" rearrange (PyanNet.py:179)
// LENS: frames t >= row_T[b] are +0, and P is not read there.
template <bool LENS>
__global__ __launch_bounds__(256) void sinc_out_kernel(const float *P, const float *scale, const float *shift, int B, int C, int L, float slope,
                                                       float *feats, int ldf, SincRowTArg<LENS> row_T) {
    const long long n = (long long)B * L * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long bt = i / C;
        const int t = (int)(bt % L), b = (int)(bt / L);
        if constexpr (LENS) {
            if (t >= row_T[b]) { feats[((size_t)b * L + t) * ldf + c] = 0.f; continue; }
        }
        float v = __builtin_fmaf(P[((size_t)b * C + c) * L + t], scale[(size_t)b * C + c], shift[(size_t)b * C + c]);
        v = v >= 0.f ? v : v * slope;
        feats[((size_t)b * L + t) * ldf + c] = v;
    }
}

// Per-row geometry of a lens call (SincGeoArgs): one workgroup; thread t takes a contiguous run of rows, the six tile counts are scanned
// across the workgroup (Hillis-Steele in LDS) and each thread writes its rows' exclusive prefixes.  The floor chain is sinc_carve's.
constexpr int GEO_THR = 1024;
__global__ __launch_bounds__(GEO_THR) void sinc_row_geometry_kernel(SincGeoArgs g) {
    __shared__ int scan[2][6][GEO_THR];
    const int tid = threadIdx.x, ld = g.B + 1;
    const int per = (g.B + GEO_THR - 1) / GEO_THR, r0 = tid * per < g.B ? tid * per : g.B, r1 = r0 + per < g.B ? r0 + per : g.B;
    int *T = g.geo;
    auto arr = [&](int stage, int k) { return g.geo + (size_t)(1 + 6 * stage + k) * ld; };   // k: 0 Lin, 1 Lpool, 2 / 3 split tiles / prefix, 4 / 5 exact
    int own[6] = {0, 0, 0, 0, 0, 0};
    for (int b = r0; b < r1; ++b) {
        long long n = g.nsamp[b];
        n = n < 0 ? 0 : n > g.S ? g.S : n;
        long long lin[3], lpool[3], L = n;
        for (int i = 0; i < 3; ++i) {
            const int st = i == 0 ? g.stride0 : 1;
            lin[i] = L;
            const long long lconv = L >= g.kw[i] ? (L - g.kw[i]) / st + 1 : 0;
            lpool[i] = lconv / 3;
            L = lpool[i];
        }
        const bool any = lpool[2] > 0;   // a row without frames is not touched by any stage
        T[b] = any ? (int)lpool[2] : 0;
        for (int i = 0; i < 3; ++i) {
            const int lp = any ? (int)lpool[i] : 0;
            const int t16 = (lp + 63) / 64, t32 = (lp + g.pt[i] - 1) / g.pt[i];
            arr(i, 0)[b] = any ? (int)lin[i] : 0;
            arr(i, 1)[b] = lp;
            arr(i, 2)[b] = t16;
            arr(i, 4)[b] = t32;
            own[2 * i] += t16;
            own[2 * i + 1] += t32;
        }
    }
    int src = 0;
    for (int k = 0; k < 6; ++k) scan[0][k][tid] = own[k];
    __syncthreads();
    for (int d = 1; d < GEO_THR; d <<= 1) {   // inclusive scan of the per-thread sums
        for (int k = 0; k < 6; ++k) scan[src ^ 1][k][tid] = scan[src][k][tid] + (tid >= d ? scan[src][k][tid - d] : 0);
        src ^= 1;
        __syncthreads();
    }
    for (int i = 0; i < 3; ++i)
        for (int f = 0; f < 2; ++f) {
            const int k = 2 * i + f;
            int run = scan[src][k][tid] - own[k];
            int *cnt = arr(i, 2 + 2 * f), *pre = arr(i, 3 + 2 * f);
            for (int b = r0; b < r1; ++b) { pre[b] = run; run += cnt[b]; }
            if (tid == GEO_THR - 1) pre[g.B] = scan[src][k][tid];
        }
}

}  // namespace

static int sinc_window(const SincConvArgs &a, int waves) { return (waves * 32 - 1) * a.stride + a.Kw; }

size_t sinc_conv_lds_bytes(const SincConvArgs &a, int NT, int waves) {
    const int NW = NT * 32;
    size_t xy = (size_t)a.Cin * sinc_window(a, waves) + 8 + 1;
    if (xy < (size_t)NW * YS) xy = (size_t)NW * YS;
    return ((size_t)a.Kp * NW + xy) * sizeof(float) + 96 * sizeof(float2);   // + the static (scale, shift) table
}

// elements of the input window each thread carries in registers between tiles
int sinc_conv_ept(const SincConvArgs &a, int waves) { return (a.Cin * sinc_window(a, waves) + waves * 64 - 1) / (waves * 64); }

// Workgroup shape of a stage: 8 waves (two per SIMD, 255 positions = 85 pooled outputs per tile) when the filter
// matrix + window fit the LDS and the window fits the register staging -- the single-channel sinc stage --
// 4 waves for the multi-channel stages under the same conditions, else 3 waves (96 positions = 32 pooled outputs).
SincConvPlan sinc_conv_plan(const SincConvArgs &a) {
    const int NT = (a.Cout + 31) / 32;
    SincConvPlan p;
    const bool wide = a.Cin == 1 && sinc_conv_lds_bytes(a, NT, 8) <= (size_t)160 * 1024 && sinc_conv_ept(a, 8) <= 8;
    // multi-channel stages: 4 waves (one per SIMD, 126 positions = 42 pooled outputs) when the wider window still fits
    const bool four = a.Cin > 1 && sinc_conv_lds_bytes(a, NT, 4) <= (size_t)160 * 1024 && sinc_conv_ept(a, 4) <= 48;
    p.waves = wide ? 8 : four ? 4 : 3;
    p.pt = p.waves * 32 / 3;
    p.phases = (p.waves + 2) / 3;
    return p;
}

hipError_t launch_wav_stats(const float *wav, int B, long long S, long long row_stride, const float *gamma, const float *beta, float eps,
                            float *scale, float *shift, hipStream_t s, const int *row_n) {
    if (row_n) hipLaunchKernelGGL(wav_stats_kernel<true>, dim3(B), dim3(1024), 0, s, wav, S, row_stride, gamma, beta, eps, scale, shift, row_n);
    else hipLaunchKernelGGL(wav_stats_kernel<false>, dim3(B), dim3(1024), 0, s, wav, S, row_stride, gamma, beta, eps, scale, shift, SincNoRows{});
    return hipGetLastError();
}

hipError_t launch_wav_stats(const int16_t *wav, int B, long long S, long long row_stride, const float *gamma, const float *beta, float eps,
                            float *scale, float *shift, hipStream_t s, const int *row_n) {
    if (row_n) hipLaunchKernelGGL(wav_stats_i16_kernel<true>, dim3(B), dim3(1024), 0, s, wav, S, row_stride, gamma, beta, eps, scale, shift, row_n);
    else hipLaunchKernelGGL(wav_stats_i16_kernel<false>, dim3(B), dim3(1024), 0, s, wav, S, row_stride, gamma, beta, eps, scale, shift, SincNoRows{});
    return hipGetLastError();
}

hipError_t launch_sinc_row_geometry(const SincGeoArgs &g, hipStream_t s) {
    if (g.B <= 0 || !g.nsamp || !g.geo) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sinc_row_geometry_kernel, dim3(1), dim3(GEO_THR), 0, s, g);
    return hipGetLastError();
}

hipError_t launch_sinc_conv(const SincConvArgs &a, hipStream_t s, const SincRows *rows) {
    const int NT = (a.Cout + 31) / 32;
    if (NT != 2 && NT != 3) return hipErrorInvalidValue;
    const SincConvPlan plan = sinc_conv_plan(a);
    if (a.ntiles != (a.Lpool + plan.pt - 1) / plan.pt) return hipErrorInvalidValue;   // the caller sized the partials with the same plan
    // the dynamic part only: sinc_conv_lds_bytes counts the static (scale, shift) table too, and the kernel's total (dynamic + static) is
    // what must fit the 160 KiB (requesting the whole figure as dynamic LDS failed the launch of stages within 768 bytes of the limit)
    const size_t lds = sinc_conv_lds_bytes(a, NT, plan.waves) - 96 * sizeof(float2);
    // persistent workgroups, one per CU (the LDS-resident filter matrix allows no more), each walking a contiguous
    // range of the (utterance, tile) pairs
    const long long total = (long long)a.B * a.ntiles;
    const int ncu = a.n_cu > 0 ? a.n_cu : 256;
    const dim3 grid((unsigned)(total < ncu ? total : ncu)), block(plan.waves * 64);
    const bool cin1 = a.Cin == 1;
    const int ept = sinc_conv_ept(a, plan.waves);
    if (ept > 48 || (cin1 && ept > 8)) return hipErrorInvalidValue;   // uvad_sincnet_configure rejects these geometries
    if (a.in_i16 && !cin1) return hipErrorInvalidValue;               // int16 is the waveform: the single-channel stage only
    const bool i16 = a.in_i16 != nullptr;
#define UVAD_SINC_LAUNCH_L(NT_, C1_, EPT_, W_, I16_, L_, ROWS_)                                                            \
    {                                                                                                                      \
        auto k = conv_pool_kernel<NT_, C1_, EPT_, W_, I16_, L_>;                                                           \
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e;                                                                                     \
        hipLaunchKernelGGL(k, grid, block, lds, s, ROWS_);                                                                 \
    }
    SincLensArgs<SincConvArgs> la{};
    static_cast<SincConvArgs &>(la) = a;
    if (rows) la.rows = *rows;
#define UVAD_SINC_LAUNCH_T(NT_, C1_, EPT_, W_, I16_) \
    { if (rows) UVAD_SINC_LAUNCH_L(NT_, C1_, EPT_, W_, I16_, true, la) else UVAD_SINC_LAUNCH_L(NT_, C1_, EPT_, W_, I16_, false, a) }
#define UVAD_SINC_LAUNCH(NT_, C1_, EPT_, W_) UVAD_SINC_LAUNCH_T(NT_, C1_, EPT_, W_, false)
#define UVAD_SINC_LAUNCH1(NT_, W_) { if (i16) UVAD_SINC_LAUNCH_T(NT_, true, 8, W_, true) else UVAD_SINC_LAUNCH_T(NT_, true, 8, W_, false) }
    if (cin1 && plan.waves == 8) {
        if (NT == 3) UVAD_SINC_LAUNCH1(3, 8) else UVAD_SINC_LAUNCH1(2, 8)
    } else if (cin1) {
        if (NT == 3) UVAD_SINC_LAUNCH1(3, 3) else UVAD_SINC_LAUNCH1(2, 3)
    } else if (plan.waves == 4) {
        if (ept <= 32) { if (NT == 3) UVAD_SINC_LAUNCH(3, false, 32, 4) else UVAD_SINC_LAUNCH(2, false, 32, 4) }
        else { if (NT == 3) UVAD_SINC_LAUNCH(3, false, 48, 4) else UVAD_SINC_LAUNCH(2, false, 48, 4) }
    } else if (ept <= 32) {
        if (NT == 3) UVAD_SINC_LAUNCH(3, false, 32, 3) else UVAD_SINC_LAUNCH(2, false, 32, 3)
    } else {
        if (NT == 3) UVAD_SINC_LAUNCH(3, false, 48, 3) else UVAD_SINC_LAUNCH(2, false, 48, 3)
    }
#undef UVAD_SINC_LAUNCH1
#undef UVAD_SINC_LAUNCH
#undef UVAD_SINC_LAUNCH_T
#undef UVAD_SINC_LAUNCH_L
    return hipGetLastError();
}

hipError_t launch_norm_finalize(const float *partials, int B, int ntiles, int pt, int phases, int NW, int C, int L, const float *gamma,
                                const float *beta, float eps, float *scale, float *shift, hipStream_t s, const SincRows *rows) {
    if (rows)
        hipLaunchKernelGGL(norm_finalize_kernel<true>, dim3(B), dim3(128), 0, s, partials, ntiles, pt, phases, NW, C, L, gamma, beta, eps, scale, shift,
                           *rows);
    else
        hipLaunchKernelGGL(norm_finalize_kernel<false>, dim3(B), dim3(128), 0, s, partials, ntiles, pt, phases, NW, C, L, gamma, beta, eps, scale, shift,
                           SincNoRows{});
    return hipGetLastError();
}

hipError_t launch_sinc_out(const float *P, const float *scale, const float *shift, int B, int C, int L, float slope, float *feats, int ldf,
                           hipStream_t s, const int *row_T) {
    const long long n = (long long)B * L * C;
    if (n <= 0) return hipSuccess;
    long long g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    if (row_T) hipLaunchKernelGGL(sinc_out_kernel<true>, dim3((int)g), dim3(256), 0, s, P, scale, shift, B, C, L, slope, feats, ldf, row_T);
    else hipLaunchKernelGGL(sinc_out_kernel<false>, dim3((int)g), dim3(256), 0, s, P, scale, shift, B, C, L, slope, feats, ldf, SincNoRows{});
    return hipGetLastError();
}

}  // namespace uvad
