// ingest.hip -- the ingest stage (uvad_ingest*, include/uvad.h): audio as it arrives -> [rows][samples] f32 at 16 kHz.
//
// One kernel serves the dense, ragged and stream forms.  A workgroup owns one source row b and a tile of TJ output groups j of ALL its
// channels (output sample o = j up + p):
//   1. taps[up][K] go to LDS; a stream's tile 0 also fetches the row's history (H decoded samples per channel) and its "output groups
//      since the session's start" counter, both read as zero under UVAD_SLOT_START;
//   2. the interleaved input frames the tile needs, [j0 down - shift, j0 down - shift + (TJ - 1) down + K), are read in memory order
//      (coalesced), decoded (G.711 by arithmetic, exact) and de-interleaved into xs[c][frame]; frames at or past the row's count are
//      never read and count as zero, frames before 0 come from the history (stream) or are zero;
//   3. a stream's tile 0 writes the next history (the last H samples of [history | chunk]) and the counter -- every read of either
//      happened in step 1, and no other workgroup touches them (a tile spans at least H input frames, so only tile 0 reaches back);
//   4. every lane computes four consecutive outputs of one channel, each its own f32 fma chain over k = 0 .. K - 1 from +0 -- the order
//      is the contract that makes the three forms agree bit for bit -- and stores them as one 16-byte vector where the row allows.
// LDS is accessed with 32-bit operations only (tests/test_abi_ingest.py), as the other kernels that run beside the MFMA kernels.
#include "../../include/uvad.h"
#include "uvad_internal.h"

namespace uvad {

namespace {

constexpr int INGEST_THREADS = 256;
constexpr int INGEST_TILE_OUT = 1024;        // outputs per channel and tile: four per lane
constexpr size_t INGEST_LDS_SOFT = 48 << 10, INGEST_LDS_HARD = 64 << 10;

// ITU-T G.711 expansion to the standard 16-bit value
__device__ __forceinline__ int ulaw_decode(unsigned u) {
    u = ~u & 0xffu;
    const int t = (int)(((u & 0x0fu) << 3) + 0x84u) << ((u & 0x70u) >> 4);
    return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
__device__ __forceinline__ int alaw_decode(unsigned a) {
    a = (a ^ 0x55u) & 0xffu;
    int t = (int)(a & 0x0fu) << 4;
    const int seg = (int)(a & 0x70u) >> 4;
    if (seg == 0) t += 8;
    else t = (t + 0x108) << (seg - 1);
    return (a & 0x80u) ? t : -t;
}
__device__ __forceinline__ float ingest_load(const void *in, int enc, size_t i) {
    switch (enc) {
    case UVAD_INGEST_F32: return static_cast<const float *>(in)[i];
    case UVAD_INGEST_I16: return (float)static_cast<const int16_t *>(in)[i] * (1.0f / 32768.0f);
    case UVAD_INGEST_ULAW: return (float)ulaw_decode(static_cast<const uint8_t *>(in)[i]) * (1.0f / 32768.0f);
    default: return (float)alaw_decode(static_cast<const uint8_t *>(in)[i]) * (1.0f / 32768.0f);
    }
}

struct IngestTile { int TJ, tiles; size_t lds; };

int round4(int v) { return (v + 3) / 4 * 4; }

size_t ingest_lds(const IngestArgs &a, int TJ) {
    const size_t span = (size_t)(TJ - 1) * a.down + a.K;
    return ((size_t)a.C * span + (size_t)a.up * a.K + (size_t)a.C * (a.hist ? a.H : 0) + a.C) * sizeof(float);
}

IngestTile ingest_tiling(const IngestArgs &a) {
    IngestTile t{};
    // a tile spans at least H input frames (only tile 0 reaches the history) and a whole number of 16-byte output vectors
    const int min_tj = round4(a.hist && a.H > 0 ? (a.H + a.down - 1) / a.down : 1);
    int TJ = round4((INGEST_TILE_OUT + a.up - 1) / a.up);
    if (TJ < min_tj) TJ = min_tj;
    while (ingest_lds(a, TJ) > INGEST_LDS_SOFT && TJ > 4 && round4(TJ / 2) >= min_tj) TJ = round4(TJ / 2);
    if (ingest_lds(a, TJ) > INGEST_LDS_HARD) return t;
    const long long groups = (a.S_out + a.up - 1) / a.up;
    const long long tiles = groups > 0 ? (groups + TJ - 1) / TJ : 1;
    if (tiles * a.B > 0x7fffffffLL) return t;
    t.TJ = TJ; t.tiles = (int)tiles; t.lds = ingest_lds(a, TJ);
    return t;
}

template <int UP>
__global__ __launch_bounds__(INGEST_THREADS) void ingest_kernel(IngestArgs a, int TJ, int tiles) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int C = a.C, K = a.K, down = a.down, H = a.hist ? a.H : 0;
    const int up = UP ? UP : a.up;
    const int span = (TJ - 1) * down + K;
    float *xs = lds;                                      // [C][span]
    float *ts = xs + C * span;                            // [up][K]
    float *hs = ts + up * K;                              // [C][H]: the history as the step found it
    int *sp = reinterpret_cast<int *>(hs + C * H);        // [C]: output groups before this step, saturated at Dj
    const bool head = a.hist != nullptr && tile == 0;
    const int shift = a.hist ? H : a.width;
    const long long j0 = (long long)tile * TJ;
    const long long f0 = j0 * down - shift;               // the tile's first input frame
    long long n = a.S_in;
    if (a.nsamp) {
        n = a.nsamp[b];
        n = n < 0 ? 0 : (n > a.S_in ? a.S_in : n);
    }
    const size_t in_row = (size_t)b * (size_t)a.S_in * C;

    // 1. taps, history, counters
    for (int i = tid; i < up * K; i += INGEST_THREADS) ts[i] = a.taps ? a.taps[i] : 1.0f;
    if (head) {
        for (int i = tid; i < C * H; i += INGEST_THREADS) {
            const int c = i / H;
            const size_t row = (size_t)b * C + c;
            const bool start = a.flags && (a.flags[row] & UVAD_SLOT_START);
            hs[i] = start ? 0.0f : a.hist[row * H + (i - c * H)];
        }
        if (tid < C) {
            const size_t row = (size_t)b * C + tid;
            const bool start = a.flags && (a.flags[row] & UVAD_SLOT_START);
            const long long s = start ? 0 : a.seen[row];
            sp[tid] = (int)(s < 0 ? 0 : (s > a.Dj ? a.Dj : s));
        }
    }
    __syncthreads();

    // 2. the tile's input frames, in memory order
    for (int e = tid; e < span * C; e += INGEST_THREADS) {
        const int fl = e / C, c = e - fl * C;
        const long long f = f0 + fl;
        float v = 0.0f;
        if (f >= 0) {
            if (f < n) v = ingest_load(a.in, a.enc, in_row + (size_t)f * C + c);
        } else if (head) {
            v = hs[c * H + (int)(H + f)];
        }
        xs[c * span + fl] = v;
    }
    __syncthreads();

    // 3. the next history and counter (a stream's n is its chunk)
    if (head) {
        for (int i = tid; i < C * H; i += INGEST_THREADS) {
            const int c = i / H, q = i - c * H;
            const long long f = a.S_in + q - H;
            a.hist[((size_t)b * C + c) * H + q] = f >= 0 ? ingest_load(a.in, a.enc, in_row + (size_t)f * C + c) : hs[c * H + (int)(H + f)];
        }
        if (tid < C) {
            const long long s = (long long)sp[tid] + a.S_in / down;
            a.seen[(size_t)b * C + tid] = s > a.Dj ? a.Dj : s;
        }
    }
    const long long n_out = ((long long)a.up * n + down - 1) / down;   // the row's outputs: ceil(up n / down)
    if (a.out_nsamp && tile == 0 && tid < C) a.out_nsamp[(size_t)b * C + tid] = n_out;

    // 4. four consecutive outputs per lane
    const bool vec = (a.S_out & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
    const int quads = TJ * up / 4;
    for (int c = 0; c < C; ++c) {
        const float *xc = xs + c * span;
        float *orow = a.out + ((size_t)b * C + c) * (size_t)a.S_out;
        const int held = head ? a.Dj - sp[c] : 0;          // output groups of this step still inside the session's first Dj
        for (int q = tid; q < quads; q += INGEST_THREADS) {
            const int ol = 4 * q;
            const long long o = j0 * up + ol;
            if (o >= a.S_out) continue;
            float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            int jl[4];
            if (!a.taps) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { jl[i] = ol + i; y[i] = xc[jl[i]]; }
            } else if (UP == 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) jl[i] = ol + i;
                const float *x0 = xc + jl[0] * down, *x1 = xc + jl[1] * down, *x2 = xc + jl[2] * down, *x3 = xc + jl[3] * down;
                for (int k = 0; k < K; ++k) {
                    const float t = ts[k];
                    y[0] = __builtin_fmaf(x0[k], t, y[0]);
                    y[1] = __builtin_fmaf(x1[k], t, y[1]);
                    y[2] = __builtin_fmaf(x2[k], t, y[2]);
                    y[3] = __builtin_fmaf(x3[k], t, y[3]);
                }
            } else if (UP == 2) {
                jl[0] = jl[1] = ol / 2; jl[2] = jl[3] = ol / 2 + 1;
                const float *x0 = xc + jl[0] * down, *x2 = xc + jl[2] * down;
                for (int k = 0; k < K; ++k) {
                    const float t0 = ts[k], t1 = ts[K + k], u = x0[k], v = x2[k];
                    y[0] = __builtin_fmaf(u, t0, y[0]);
                    y[1] = __builtin_fmaf(u, t1, y[1]);
                    y[2] = __builtin_fmaf(v, t0, y[2]);
                    y[3] = __builtin_fmaf(v, t1, y[3]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    jl[i] = (ol + i) / up;
                    const float *x = xc + jl[i] * down, *t = ts + (ol + i - jl[i] * up) * K;
                    float acc = 0.0f;
                    for (int k = 0; k < K; ++k) acc = __builtin_fmaf(x[k], t[k], acc);
                    y[i] = acc;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)   // +0 past the row's count, and for a session's first Dj output groups
                if (o + i >= n_out || jl[i] < held) y[i] = 0.0f;
            if (vec && o + 3 < a.S_out) {
                *reinterpret_cast<float4 *>(orow + o) = make_float4(y[0], y[1], y[2], y[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (o + i < a.S_out) orow[o + i] = y[i];
            }
        }
    }
}

}  // namespace

hipError_t launch_ingest(const IngestArgs &a, hipStream_t s) {
    if (!a.in || a.B <= 0 || a.C < 1 || a.C > INGEST_MAX_CHANNELS || a.S_in < 0 || a.S_out < 0 || (a.S_out > 0 && !a.out)) return hipErrorInvalidValue;
    if (a.enc < UVAD_INGEST_F32 || a.enc > UVAD_INGEST_ALAW) return hipErrorInvalidValue;
    if (a.up < 1 || a.up > INGEST_MAX_PHASES || a.down < 1 || a.K < 1 || a.K > INGEST_MAX_TAPS || a.width < 0) return hipErrorInvalidValue;
    if (a.taps ? a.K != 2 * a.width + a.down : (a.up != 1 || a.down != 1 || a.K != 1 || a.width != 0)) return hipErrorInvalidValue;
    if (a.hist) {   // a stream step: whole output groups, the history the delay needs, no per-row counts
        if (!a.seen || a.nsamp || a.out_nsamp || a.Dj < 0 || a.H != a.Dj * a.down + a.width || a.S_in % a.down) return hipErrorInvalidValue;
        if (a.S_out != a.S_in / a.down * a.up) return hipErrorInvalidValue;
    } else if (a.S_out != (a.S_in * a.up + a.down - 1) / a.down) {
        return hipErrorInvalidValue;
    }
    if (a.S_out == 0 && !a.out_nsamp) return hipSuccess;
    const IngestTile t = ingest_tiling(a);
    if (t.TJ <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((long long)t.tiles * a.B)), block(INGEST_THREADS);
    if (a.up == 1) hipLaunchKernelGGL(ingest_kernel<1>, grid, block, t.lds, s, a, t.TJ, t.tiles);
    else if (a.up == 2) hipLaunchKernelGGL(ingest_kernel<2>, grid, block, t.lds, s, a, t.TJ, t.tiles);
    else hipLaunchKernelGGL(ingest_kernel<0>, grid, block, t.lds, s, a, t.TJ, t.tiles);
    return hipGetLastError();
}

}  // namespace uvad
