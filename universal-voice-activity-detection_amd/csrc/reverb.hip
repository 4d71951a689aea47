// reverb.hip -- reverberation of training batches on the device (uvad_reverb_*, include/uvad.h): per batch and per row, either the row as it
// is or the row convolved with one room impulse response of a device-resident bank, drawn anew for every call from the Philox stream of the
// dropout stage (philox.h).  What lhotse's reverb_rir does once on the host before features are stored.  A step is two to four launches:
//   reverb_plan_kernel       ONE workgroup: its first thread takes the draw ordinal from the state (uvad_reverb_step, advancing it) or from
//                            the caller (uvad_reverb_apply); then a thread per row draws {applied, r}, looks up d and writes the plan row
//                            {applied, r, d, bits of 1.0f} to the workspace, and to d_plan when that is given.
//   reverb_conv_kernel<fmt>  one workgroup per (row, 4096 output samples).  A row not drawn is copied (the input's bits, +0 past its length).
//                            A drawn row is the direct form on the f32 matrix cores, v_mfma_f32_32x32x2_f32 (exact f32 products, one
//                            accumulation chain): M = 32 output phases j, N = 32 output blocks i of 32 samples per wave, k = input offset s
//                            over K_r + 31 values, A[j][s] = h[s - 31 + j] straight from the response (no Toeplitz matrix anywhere),
//                            B[s][i] = x[32 i + 31 + d - s], a stride-32 Hankel window of the row.  The offsets are walked in chunks of 256:
//                            per chunk the workgroup stages h[s0 - 31 .. s0 + 255] and the 4320 samples its four waves' windows cover in
//                            LDS (zeros outside the response and outside [0, n_b), which are never read from memory), the samples padded by
//                            one word per 32 so that the stride-32 reads of the B operand hit 32 different banks.  Every output is ONE
//                            chain from +0 over s = 0, 1, .. in that order, i.e. over the taps in increasing k with zero products in front
//                            and behind: a function of (K_r, i) alone.  The work of a workgroup is bounded by (n_b, K_r): a tile at or past
//                            n_b only writes zeros, a wave whose 1024 outputs start past n_b issues no product.
//                            This is the plain form: no double buffering of the stages, one accumulator tile per wave, scalar stores.
//   reverb_gain_kernel<fmt>  (normalize) one workgroup of 1024 lanes per drawn row: E_in and E_out in the order of the mix stage
//                            (energy_order.h), g = (float)sqrt(E_in / E_out) in double, into the plan.
//   reverb_scale_kernel      (normalize) out = fl32(z g) over the drawn rows.
// uvad_reverb_reset runs reverb_delay_kernel, one workgroup per response: the smallest k at which |h[k]| is largest, a NaN never winning.
// Nothing is summed across workgroups and nothing is contracted (the Makefile's flag): the same call gives the same bits, and tests/reverb_ref.py restates it.
#include "../../include/uvad.h"
#include "energy_order.h"
#include "philox.h"
#include "uvad_internal.h"

namespace uvad {

static_assert(sizeof(ReverbHeader) == 256, "state layout");
static_assert(offsetof(ReverbHeader, thr) == 16 && offsetof(ReverbHeader, seed) == 24 && offsetof(ReverbHeader, bank_total) == 32 &&
              offsetof(ReverbHeader, max_taps) == 40 && offsetof(ReverbHeader, draws) == 56, "the header of include/uvad.h");
static_assert(REVERB_PLAN_WORDS == UVAD_REVERB_PLAN_WORDS && REVERB_MAX_TAPS == UVAD_REVERB_MAX_TAPS && REVERB_TILE == UVAD_REVERB_TILE &&
              REVERB_KC == UVAD_REVERB_K_CHUNK, "the constants of include/uvad.h");

static size_t reverb_pad(size_t v) { return (v + 255) / 256 * 256; }

ReverbLayout reverb_layout(int n_rirs) {
    ReverbLayout l{};
    l.off_first = sizeof(ReverbHeader);
    l.off_taps = l.off_first + reverb_pad(((size_t)n_rirs + 1) * 8);
    l.off_delay = l.off_taps + reverb_pad((size_t)n_rirs * 4);
    l.total = l.off_delay + reverb_pad((size_t)n_rirs * 4);
    return l;
}

size_t reverb_ws_bytes(int B) { return sizeof(MixWsHead) + reverb_pad((size_t)B * REVERB_PLAN_WORDS * 4); }

namespace {

constexpr int RV_THREADS = 256, RV_WAVE_TILE = REVERB_TILE / 4;
constexpr int RV_WIN = REVERB_TILE + REVERB_KC - 32;           // samples the four waves' windows cover in one chunk of offsets
constexpr int RV_XS = RV_WIN + RV_WIN / 32 + 1;                // ... padded by one word per 32
static_assert(REVERB_KC % 32 == 0 && RV_WAVE_TILE == 32 * 32, "a wave owns 32 blocks of 32 phases");

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int FMT>
__device__ __forceinline__ float rv_load(const void *row, long long i) {
    if constexpr (FMT == UVAD_INGEST_F32) return reinterpret_cast<const float *>(row)[i];
    else return (float)reinterpret_cast<const short *>(row)[i] * (1.0f / 32768.0f);
}

template <int FMT>
__device__ __forceinline__ const void *rv_row(const void *in, long long b, long long S) {
    return FMT == UVAD_INGEST_F32 ? static_cast<const void *>(reinterpret_cast<const float *>(in) + b * S)
                                  : static_cast<const void *>(reinterpret_cast<const short *>(in) + b * S);
}

__global__ __launch_bounds__(RV_THREADS) void reverb_delay_kernel(const float *bank, const long long *first, const int *taps, int *delay) {
    __shared__ float s_v[RV_THREADS];
    __shared__ int s_i[RV_THREADS];
    const int r = blockIdx.x, t = threadIdx.x, K = taps[r];
    const float *h = bank + first[r];
    float best = -1.0f;                                         // below every |h|: tap 0 wins a response of zeros, and one of NaNs
    int bi = 0;
    for (int k = t; k < K; k += RV_THREADS) {                   // increasing k: `>` keeps the smallest; a NaN compares false
        const float v = __builtin_fabsf(h[k]);
        if (v > best) { best = v; bi = k; }
    }
    s_v[t] = best; s_i[t] = bi;
    __syncthreads();
    for (int o = RV_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) {
            const float v = s_v[t + o];
            const int i = s_i[t + o];
            if (v > s_v[t] || (v == s_v[t] && i < s_i[t])) { s_v[t] = v; s_i[t] = i; }
        }
        __syncthreads();
    }
    if (t == 0) delay[r] = s_i[0];
}

struct ReverbPlanArgs {
    int B; ReverbHeader *state; const int *delay; MixWsHead *head; int *plan; int *user_plan;
    int take; unsigned long long draw; long long row0;
};

__global__ __launch_bounds__(RV_THREADS) void reverb_plan_kernel(ReverbPlanArgs a) {
    __shared__ unsigned s_draw[2];
    if (threadIdx.x == 0) {                                     // the one writer of the ordinal
        unsigned long long d = a.draw;
        if (a.take) {                                           // (a state that lost its magic draws nothing: no row is reverberated)
            d = a.state->draws;
            a.state->draws = d + 1;
        }
        a.head->draw = d; a.head->row0 = a.row0;
        s_draw[0] = (unsigned)d; s_draw[1] = (unsigned)(d >> 32);
    }
    __syncthreads();
    const ReverbHeader &hd = *a.state;
    const bool ok = hd.magic == REVERB_MAGIC && hd.n_rirs >= 1;
    const unsigned long long seed = hd.seed;
    for (int b = threadIdx.x; b < a.B; b += RV_THREADS) {
        const unsigned row = (unsigned)(a.row0 + b);
        const uint4 w = lt_philox(make_uint4(row, 0x52560000u, s_draw[0], s_draw[1]), (unsigned)seed, (unsigned)(seed >> 32));
        const bool applied = ok && (unsigned long long)w.x < hd.thr;
        const int r = applied ? (int)(((unsigned long long)w.y * (unsigned)hd.n_rirs) >> 32) : 0;
        const int d = applied && hd.align ? a.delay[r] : 0;
        const int one = __float_as_int(1.0f);
        int *p = a.plan + (size_t)b * REVERB_PLAN_WORDS;
        p[0] = applied ? 1 : 0; p[1] = r; p[2] = d; p[3] = one;
        if (a.user_plan) {
            int *up = a.user_plan + (size_t)b * REVERB_PLAN_WORDS;
            up[0] = p[0]; up[1] = r; up[2] = d; up[3] = one;
        }
    }
}

struct ReverbConvArgs {
    const void *in; float *out; long long S, tiles; const long long *nsamp;
    const int *plan; const float *bank; const long long *first; const int *taps;
};

template <int FMT>
__global__ __launch_bounds__(RV_THREADS) void reverb_conv_kernel(ReverbConvArgs a) {
    __shared__ float hs[REVERB_KC + 32];
    __shared__ float xs[RV_XS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x / a.tiles, t0 = (blockIdx.x - b * a.tiles) * REVERB_TILE;
    const long long n = mix_row_len(a.nsamp, b, a.S);
    const int *p = a.plan + (size_t)b * REVERB_PLAN_WORDS;
    const void *row = rv_row<FMT>(a.in, b, a.S);
    float *orow = a.out + b * a.S;
    if (!p[0] || t0 >= n) {                                     // a copy (the input's bits), or the zeros past a length: block-uniform
#pragma unroll
        for (int u = 0; u < REVERB_TILE / RV_THREADS; ++u) {
            const long long i = t0 + u * RV_THREADS + tid;
            if (i < a.S) orow[i] = i < n ? rv_load<FMT>(row, i) : 0.0f;
        }
        return;
    }
    const int r = p[1], d = p[2], K = a.taps[r];
    const float *h = a.bank + a.first[r];
    const int jn = lane & 31, half = lane >> 5, il = wave * 32 + jn;
    const long long wt0 = t0 + (long long)wave * RV_WAVE_TILE;
    const bool active = wt0 < n;                                // wave-uniform
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    const int s_end = K + 31;                                   // offsets s = 0 .. K + 30: h index s - 31 + j covers every tap for every phase
    for (int s0 = 0; s0 < s_end; s0 += REVERB_KC) {
        __syncthreads();                                        // the previous chunk's readers are done
        for (int e = tid; e < REVERB_KC + 31; e += RV_THREADS) {
            const int k = s0 - 31 + e;
            hs[e] = k >= 0 && k < K ? h[k] : 0.0f;
        }
        const long long wb = t0 + d - s0 - REVERB_KC + 32;      // the row sample at window position 0
        for (int w = tid; w < RV_WIN; w += RV_THREADS) {
            const long long xi = wb + w;
            xs[w + (w >> 5)] = xi >= 0 && xi < n ? rv_load<FMT>(row, xi) : 0.0f;
        }
        __syncthreads();
        if (active) {
            const int kmax = s_end - s0 < REVERB_KC ? s_end - s0 : REVERB_KC;
            for (int kk = 0; kk < kmax; kk += 2) {             // s = s0 + kk + half: window position 32 il + (KC - 1 - (kk + half))
                const int kl = kk + half, q = REVERB_KC - 1 - kl;
                const float av = hs[kl + jn];
                const float bv = xs[33 * il + q + (q >> 5)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
        }
    }
    // C / D map of the 32 x 32 shapes: column (block) = lane & 31, row (phase) = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
    if (active) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const long long i = wt0 + 32 * jn + (q & 3) + 8 * (q >> 2) + 4 * half;
            if (i < n) orow[i] = acc[q];
        }
    }
#pragma unroll
    for (int u = 0; u < REVERB_TILE / RV_THREADS; ++u) {        // the tile's samples past the length
        const long long i = t0 + u * RV_THREADS + tid;
        if (i >= n && i < a.S) orow[i] = 0.0f;
    }
}

struct ReverbGainArgs { const void *in; const float *out; long long S; const long long *nsamp; int *plan; int *user_plan; };

template <int FMT>
__global__ __launch_bounds__(MIX_LANES) void reverb_gain_kernel(ReverbGainArgs a) {
    __shared__ int s_lo[MIX_LANES / 64], s_hi[MIX_LANES / 64];
    const long long b = blockIdx.x;
    int *p = a.plan + (size_t)b * REVERB_PLAN_WORDS;
    if (!p[0]) return;                                          // block-uniform
    const long long n = mix_row_len(a.nsamp, b, a.S);
    const double w_in = mix_energy_sum<FMT>(rv_row<FMT>(a.in, b, a.S), n, s_lo, s_hi);
    __syncthreads();                                            // the partial sums of the input are read
    const double w_out = mix_energy_sum<UVAD_INGEST_F32>(a.out + b * a.S, n, s_lo, s_hi);
    if (threadIdx.x == 0) {
        const double e_in = n > 0 ? w_in / (double)n : 0.0, e_out = n > 0 ? w_out / (double)n : 0.0;
        float g = 1.0f;
        if (e_in != 0.0 && e_out != 0.0) g = (float)__builtin_sqrt(e_in / e_out);
        p[3] = __float_as_int(g);
        if (a.user_plan) a.user_plan[(size_t)b * REVERB_PLAN_WORDS + 3] = __float_as_int(g);
    }
}

__global__ __launch_bounds__(RV_THREADS) void reverb_scale_kernel(float *out, long long S, long long tiles, const long long *nsamp, const int *plan) {
    const long long b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * REVERB_TILE;
    const int *p = plan + (size_t)b * REVERB_PLAN_WORDS;
    const long long n = mix_row_len(nsamp, b, S);
    if (!p[0] || t0 >= n) return;
    const float g = __int_as_float(p[3]);
    float *orow = out + b * S;
#pragma unroll
    for (int u = 0; u < REVERB_TILE / RV_THREADS; ++u) {
        const long long i = t0 + u * RV_THREADS + threadIdx.x;
        if (i < n) orow[i] = orow[i] * g;
    }
}

}  // namespace

hipError_t launch_reverb_delays(const float *bank, void *state, int n_rirs, hipStream_t s) {
    if (!bank || !state || n_rirs < 1) return hipErrorInvalidValue;
    const ReverbLayout l = reverb_layout(n_rirs);
    char *base = reinterpret_cast<char *>(state);
    hipLaunchKernelGGL(reverb_delay_kernel, dim3((unsigned)n_rirs), dim3(RV_THREADS), 0, s, bank, reinterpret_cast<const long long *>(base + l.off_first),
                       reinterpret_cast<const int *>(base + l.off_taps), reinterpret_cast<int *>(base + l.off_delay));
    return hipGetLastError();
}

hipError_t launch_reverb(const ReverbArgs &a, hipStream_t s) {
    if (!a.in || !a.out || !a.bank || !a.state || !a.ws || a.B < 1 || a.S < 1 || a.S > MIX_MAX_S || a.n_rirs < 1 ||
        (a.fmt != UVAD_INGEST_F32 && a.fmt != UVAD_INGEST_I16) || a.in == static_cast<const void *>(a.out))
        return hipErrorInvalidValue;
    const long long tiles = (a.S + REVERB_TILE - 1) / REVERB_TILE;
    if ((long long)a.B * tiles > 2147483647LL) return hipErrorInvalidValue;
    const ReverbLayout l = reverb_layout(a.n_rirs);
    char *st = reinterpret_cast<char *>(a.state), *ws = reinterpret_cast<char *>(a.ws);
    int *plan = reinterpret_cast<int *>(ws + sizeof(MixWsHead));
    const bool f32 = a.fmt == UVAD_INGEST_F32;
    const unsigned blocks = (unsigned)((long long)a.B * tiles);

    ReverbPlanArgs q{};
    q.B = a.B; q.state = reinterpret_cast<ReverbHeader *>(st); q.delay = reinterpret_cast<const int *>(st + l.off_delay);
    q.head = reinterpret_cast<MixWsHead *>(ws); q.plan = plan; q.user_plan = a.plan; q.take = a.take ? 1 : 0; q.draw = a.draw; q.row0 = a.row0;
    hipLaunchKernelGGL(reverb_plan_kernel, dim3(1), dim3(RV_THREADS), 0, s, q);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;

    ReverbConvArgs c{};
    c.in = a.in; c.out = a.out; c.S = a.S; c.tiles = tiles; c.nsamp = a.nsamp; c.plan = plan; c.bank = a.bank;
    c.first = reinterpret_cast<const long long *>(st + l.off_first); c.taps = reinterpret_cast<const int *>(st + l.off_taps);
    if (f32) hipLaunchKernelGGL(reverb_conv_kernel<UVAD_INGEST_F32>, dim3(blocks), dim3(RV_THREADS), 0, s, c);
    else hipLaunchKernelGGL(reverb_conv_kernel<UVAD_INGEST_I16>, dim3(blocks), dim3(RV_THREADS), 0, s, c);
    err = hipGetLastError();
    if (err != hipSuccess || !a.normalize) return err;

    ReverbGainArgs g{};
    g.in = a.in; g.out = a.out; g.S = a.S; g.nsamp = a.nsamp; g.plan = plan; g.user_plan = a.plan;
    if (f32) hipLaunchKernelGGL(reverb_gain_kernel<UVAD_INGEST_F32>, dim3((unsigned)a.B), dim3(MIX_LANES), 0, s, g);
    else hipLaunchKernelGGL(reverb_gain_kernel<UVAD_INGEST_I16>, dim3((unsigned)a.B), dim3(MIX_LANES), 0, s, g);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(reverb_scale_kernel, dim3(blocks), dim3(RV_THREADS), 0, s, a.out, a.S, tiles, a.nsamp, static_cast<const int *>(plan));
    return hipGetLastError();
}

}  // namespace uvad
