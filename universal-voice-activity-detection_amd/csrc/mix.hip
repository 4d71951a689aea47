// mix.hip -- noise mixing of training batches on the device (uvad_mix_*, include/uvad.h): what cuts.mix(noise_cuts, snr = (10, 20),
// mix_prob = 0.5) does to the training phase of every corpus recipe of the reference (src/datasets/*/utils.py), redrawn for every batch from
// the Philox stream of the dropout stage (philox.h) instead of once on the host.  A step is three launches:
//   mix_energy_kernel<fmt>   E = (sum (double)x (double)x) / n of every row, one workgroup of 1024 lanes per row in the fixed order of
//                            include/uvad.h (energy_order.h, shared with reverb.hip): lane t = (i / 4) mod 1024 adds its samples in
//                            increasing i, the lanes are folded by a tree.
//                            16-byte loads where the row starts on a 16-byte boundary (8-byte for int16), guarded dword loads elsewhere and
//                            in the group that holds the row's end; nothing at or past a length is read.  Its first thread takes the draw
//                            ordinal from the state (uvad_mix_step) or the caller (uvad_mix_apply) and records it in the workspace header.
//                            uvad_mix_reset runs the same kernel over the clips of the bank.
//   mix_plan_kernel          one thread per row: the row's draws, its segments laid end to end, the gains (double division and square root,
//                            one rounding to f32).  The plan row goes to the workspace, and to d_plan when that is given.
//   mix_pass_kernel<fmt>     out = fl(x + fl(gain noise)) inside the segments, the input's bits outside, +0 past a length: 4096-sample tiles of
//                            256 threads x 4 groups of 4 samples, a grid-stride loop over (row, tile).  The row's segments sit in LDS as 32-bit
//                            words; a group finds its segment by binary search.  The noise side starts at any sample offset: a group inside
//                            one segment reads the two aligned 16-byte words that hold its four samples and picks them by the offset's low
//                            bits; only a group that straddles a segment end or the row's length, or touches the first or last 16 bytes of
//                            the bank, goes sample by sample.  In place (f32), tiles that keep the input's bits are skipped.
// No floating-point atomics and no contraction (the Makefile's flag): the same call gives the same bits, and tests/mix_ref.py restates it.
#include "../../include/uvad.h"
#include "energy_order.h"
#include "philox.h"
#include "uvad_internal.h"

namespace uvad {

static_assert(sizeof(MixHeader) == 256 && sizeof(MixWsHead) == 256, "state and workspace layout");
static_assert(offsetof(MixHeader, thr) == 16 && offsetof(MixHeader, seed) == 24 && offsetof(MixHeader, bank_total) == 32 &&
              offsetof(MixHeader, draws) == 56, "the header of include/uvad.h");
static_assert(MIX_MAX_SEG == UVAD_MIX_MAX_SEG && MIX_PLAN_HEAD == UVAD_MIX_PLAN_HEAD && MIX_SEG_WORDS == UVAD_MIX_SEG_WORDS, "the plan record");

static size_t mix_align(size_t v) { return (v + 255) / 256 * 256; }

MixLayout mix_layout(int n_clips, int Q) {
    MixLayout l{};
    l.off_first = sizeof(MixHeader);
    l.off_energy = l.off_first + mix_align(((size_t)n_clips + 1) * 8);
    l.off_amp = l.off_energy + mix_align((size_t)n_clips * 8);
    l.total = l.off_amp + mix_align((size_t)Q * 8);
    return l;
}

MixWs mix_ws(int B, int max_seg) {
    MixWs w{};
    w.plan_words = MIX_PLAN_HEAD + MIX_SEG_WORDS * max_seg;
    w.off_energy = sizeof(MixWsHead);
    w.off_plan = w.off_energy + mix_align((size_t)B * 8);
    w.total = w.off_plan + mix_align((size_t)B * w.plan_words * 4);
    return w;
}

namespace {

constexpr int MIX_TILE = 4096, MIX_PASS_THREADS = 256, MIX_PASS_BLOCKS = 8192;

// mode 0: the clips of the bank (rows = first[b] .. first[b + 1]); 1: a step (the state's ordinal, advanced); 2: apply (the caller's draw)
struct MixEnergyArgs {
    const void *in; long long S; const long long *nsamp; const long long *first; double *energy;
    MixHeader *state; MixWsHead *head; int mode; unsigned long long draw; long long row0;
};

template <int FMT>
__global__ __launch_bounds__(MIX_LANES) void mix_energy_kernel(MixEnergyArgs a) {
    __shared__ int s_lo[MIX_LANES / 64], s_hi[MIX_LANES / 64];
    const long long b = blockIdx.x;
    const int t = threadIdx.x;
    if (a.mode && b == 0 && t == 0) {                           // the one writer of the ordinal
        unsigned long long d = a.draw;
        if (a.mode == 1) {                                      // (a state that lost its magic draws nothing: mix_plan_kernel mixes no row)
            d = a.state->draws;
            a.state->draws = d + 1;
        }
        a.head->draw = d; a.head->row0 = a.row0;
    }
    long long base, n;
    if (a.first) { base = a.first[b]; n = a.first[b + 1] - base; }
    else { base = b * a.S; n = mix_row_len(a.nsamp, b, a.S); }
    const void *row = FMT == UVAD_INGEST_F32 ? static_cast<const void *>(reinterpret_cast<const float *>(a.in) + base)
                                             : static_cast<const void *>(reinterpret_cast<const short *>(a.in) + base);
    const double w = mix_energy_sum<FMT>(row, n, s_lo, s_hi);     // energy_order.h: the order of include/uvad.h
    if (t == 0) a.energy[b] = n > 0 ? w / (double)n : 0.0;
}

struct MixPlanArgs {
    int B; long long S; const long long *nsamp;
    const MixHeader *state; const long long *first; const double *cenergy; const double *amp;
    const MixWsHead *head; const double *energy; int *plan; int *user_plan; int plan_words;
};

__global__ __launch_bounds__(64) void mix_plan_kernel(MixPlanArgs a) {
    const int b = (int)blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const MixHeader &hd = *a.state;
    int *p = a.plan + (size_t)b * a.plan_words;
    int *up = a.user_plan ? a.user_plan + (size_t)b * a.plan_words : nullptr;
    const int max_seg = (a.plan_words - MIX_PLAN_HEAD) / MIX_SEG_WORDS;
    const bool ok = hd.magic == MIX_MAGIC && hd.n_clips >= 1 && hd.Q >= 1 && hd.max_seg == max_seg;   // else: nothing is mixed
    const long long len = mix_row_len(a.nsamp, b, a.S);
    const unsigned long long draw = a.head->draw, seed = hd.seed;
    const unsigned row = (unsigned)(a.head->row0 + b);
    const uint4 w0 = lt_philox(make_uint4(row, 0u, (unsigned)draw, (unsigned)(draw >> 32)), (unsigned)seed, (unsigned)(seed >> 32));
    const bool mixed = ok && (unsigned long long)w0.x < hd.thr;
    const int q = ok ? (int)(((unsigned long long)w0.y * (unsigned)hd.Q) >> 32) : 0;
    const double e_row = a.energy[b];
    int nseg = 0;
    long long off = 0;
    if (mixed) {
        const double amp = a.amp[q];
        while (off < len && nseg < max_seg) {
            const uint4 w = nseg == 0 ? w0 : lt_philox(make_uint4(row, (unsigned)nseg, (unsigned)draw, (unsigned)(draw >> 32)), (unsigned)seed,
                                                       (unsigned)(seed >> 32));
            const int clip = (int)(((unsigned long long)w.z * (unsigned)hd.n_clips) >> 32);
            const long long cl = a.first[clip + 1] - a.first[clip];
            const long long cnt = cl < len - off ? cl : len - off;
            const double e_clip = a.cenergy[clip];
            float gain = 0.0f;
            if (e_clip != 0.0 && e_row != 0.0) gain = (float)(amp * __builtin_sqrt(e_row / e_clip));
            const int s = MIX_PLAN_HEAD + MIX_SEG_WORDS * nseg;
            const int gb = __float_as_int(gain);
            p[s] = clip; p[s + 1] = (int)off; p[s + 2] = (int)cnt; p[s + 3] = gb;
            if (up) { up[s] = clip; up[s + 1] = (int)off; up[s + 2] = (int)cnt; up[s + 3] = gb; }
            off += cnt;
            ++nseg;
        }
    }
    p[0] = mixed ? 1 : 0; p[1] = q; p[2] = nseg; p[3] = 0;
    if (up) { up[0] = p[0]; up[1] = q; up[2] = nseg; up[3] = 0; }
    for (int s = MIX_PLAN_HEAD + MIX_SEG_WORDS * nseg; s < a.plan_words; ++s) {   // unused slots read as zeros
        p[s] = 0;
        if (up) up[s] = 0;
    }
}

// four noise samples from sample `src` of the bank, src + 4 <= total
__device__ __forceinline__ float4 mix_noise4(const float *bank, long long src, long long total) {
    const float *p = bank + src;
    const unsigned r = (unsigned)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;
    if (r == 0) return *reinterpret_cast<const float4 *>(p);
    const float *pa = p - r;                                    // the 16-byte word that holds sample src, and the next one
    if (pa >= bank && src - r + 8 <= total) {
        const float4 lo = *reinterpret_cast<const float4 *>(pa), hi = *reinterpret_cast<const float4 *>(pa + 4);
        if (r == 1) return make_float4(lo.y, lo.z, lo.w, hi.x);
        if (r == 2) return make_float4(lo.z, lo.w, hi.x, hi.y);
        return make_float4(lo.w, hi.x, hi.y, hi.z);
    }
    return make_float4(p[0], p[1], p[2], p[3]);                 // the first / last 16 bytes of the bank
}

struct MixPassArgs {
    const void *in; float *out; int B; long long S, tiles; const long long *nsamp;
    const int *plan; int plan_words; const float *bank; const MixHeader *state; const long long *first; bool inplace;
};

template <int FMT>
__global__ __launch_bounds__(MIX_PASS_THREADS) void mix_pass_kernel(MixPassArgs a) {
    __shared__ int s_off[MIX_MAX_SEG], s_end[MIX_MAX_SEG], s_gain[MIX_MAX_SEG], s_src_lo[MIX_MAX_SEG], s_src_hi[MIX_MAX_SEG];
    const int t = threadIdx.x;
    const long long total = (long long)a.B * a.tiles, bank_total = a.state->bank_total;
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long b = w / a.tiles, t0 = (w - b * a.tiles) * MIX_TILE;
        const long long t1 = t0 + MIX_TILE < a.S ? t0 + MIX_TILE : a.S;
        const long long len = mix_row_len(a.nsamp, b, a.S);
        const int *p = a.plan + (size_t)b * a.plan_words;
        int nseg = p[2];
        nseg = nseg < 0 ? 0 : nseg > MIX_MAX_SEG ? MIX_MAX_SEG : nseg;
        const long long covered = nseg ? (long long)p[MIX_PLAN_HEAD + MIX_SEG_WORDS * (nseg - 1) + 1] + p[MIX_PLAN_HEAD + MIX_SEG_WORDS * (nseg - 1) + 2] : 0;
        if (a.inplace && t1 <= len && t0 >= covered) continue;   // the tile keeps the input's bits (block-uniform)
        const bool mixing = t0 < covered;
        __syncthreads();                                         // the previous tile's readers are done
        if (mixing && t < nseg) {
            const int *sg = p + MIX_PLAN_HEAD + MIX_SEG_WORDS * t;
            const long long src = a.first[sg[0]] - sg[1];        // bank index of row sample i is src + i
            s_off[t] = sg[1]; s_end[t] = sg[1] + sg[2]; s_gain[t] = sg[3];
            s_src_lo[t] = (int)(unsigned)(unsigned long long)src; s_src_hi[t] = (int)(src >> 32);
        }
        __syncthreads();
        const void *row = FMT == UVAD_INGEST_F32 ? static_cast<const void *>(reinterpret_cast<const float *>(a.in) + b * a.S)
                                                 : static_cast<const void *>(reinterpret_cast<const short *>(a.in) + b * a.S);
        float *orow = a.out + b * a.S;
        const bool vec_in = mix_row_vec<FMT>(row), vec_out = (reinterpret_cast<uintptr_t>(orow) & 15) == 0;
#pragma unroll
        for (int u = 0; u < MIX_TILE / (4 * MIX_PASS_THREADS); ++u) {
            const long long i = t0 + ((long long)u * MIX_PASS_THREADS + t) * 4;
            if (i >= a.S) continue;
            const float4 x = mix_load4<FMT>(row, i, len, vec_in);
            float xv[4] = {x.x, x.y, x.z, x.w};
            if (i < covered) {
                const int ii = (int)i;
                int k = 0;
#pragma unroll
                for (int s = MIX_MAX_SEG / 2; s > 0; s >>= 1)     // the last segment that starts at or before i
                    if (k + s < nseg && s_off[k + s] <= ii) k += s;
                if (ii + 4 <= s_end[k]) {
                    const long long src = (long long)(((unsigned long long)(unsigned)s_src_hi[k] << 32) | (unsigned)s_src_lo[k]);
                    const float4 nz = mix_noise4(a.bank, src + i, bank_total);
                    const float g = __int_as_float(s_gain[k]);
                    xv[0] = xv[0] + g * nz.x; xv[1] = xv[1] + g * nz.y; xv[2] = xv[2] + g * nz.z; xv[3] = xv[3] + g * nz.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ie = ii + e;
                        while (k < nseg - 1 && ie >= s_end[k]) ++k;
                        if (ie < s_end[k]) {                     // inside segment k: s_off[k] <= ie, and s_end[k] <= len
                            const long long src = (long long)(((unsigned long long)(unsigned)s_src_hi[k] << 32) | (unsigned)s_src_lo[k]);
                            xv[e] = xv[e] + __int_as_float(s_gain[k]) * a.bank[src + ie];
                        }
                    }
                }
            }
            if (vec_out && i + 4 <= a.S) {
                *reinterpret_cast<float4 *>(orow + i) = make_float4(xv[0], xv[1], xv[2], xv[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i + e < a.S) orow[i + e] = xv[e];
            }
        }
    }
}

}  // namespace

hipError_t launch_mix_clip_energies(const float *bank, void *state, int n_clips, int Q, hipStream_t s) {
    if (!bank || !state || n_clips < 1 || Q < 1) return hipErrorInvalidValue;
    const MixLayout l = mix_layout(n_clips, Q);
    char *base = reinterpret_cast<char *>(state);
    MixEnergyArgs e{};
    e.in = bank; e.first = reinterpret_cast<const long long *>(base + l.off_first); e.energy = reinterpret_cast<double *>(base + l.off_energy);
    e.mode = 0;
    hipLaunchKernelGGL(mix_energy_kernel<UVAD_INGEST_F32>, dim3((unsigned)n_clips), dim3(MIX_LANES), 0, s, e);
    return hipGetLastError();
}

hipError_t launch_mix(const MixArgs &a, hipStream_t s) {
    if (!a.in || !a.out || !a.bank || !a.state || !a.ws || a.B < 1 || a.S < 1 || a.S > MIX_MAX_S || a.n_clips < 1 || a.Q < 1 || a.max_seg < 1 ||
        a.max_seg > MIX_MAX_SEG || (a.fmt != UVAD_INGEST_F32 && a.fmt != UVAD_INGEST_I16))
        return hipErrorInvalidValue;
    const MixLayout l = mix_layout(a.n_clips, a.Q);
    const MixWs w = mix_ws(a.B, a.max_seg);
    char *st = reinterpret_cast<char *>(a.state), *ws = reinterpret_cast<char *>(a.ws);
    const bool f32 = a.fmt == UVAD_INGEST_F32;

    MixEnergyArgs e{};
    e.in = a.in; e.S = a.S; e.nsamp = a.nsamp; e.energy = reinterpret_cast<double *>(ws + w.off_energy);
    e.state = reinterpret_cast<MixHeader *>(st); e.head = reinterpret_cast<MixWsHead *>(ws);
    e.mode = a.take ? 1 : 2; e.draw = a.draw; e.row0 = a.row0;
    if (f32) hipLaunchKernelGGL(mix_energy_kernel<UVAD_INGEST_F32>, dim3((unsigned)a.B), dim3(MIX_LANES), 0, s, e);
    else hipLaunchKernelGGL(mix_energy_kernel<UVAD_INGEST_I16>, dim3((unsigned)a.B), dim3(MIX_LANES), 0, s, e);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;

    MixPlanArgs q{};
    q.B = a.B; q.S = a.S; q.nsamp = a.nsamp;
    q.state = reinterpret_cast<const MixHeader *>(st); q.first = reinterpret_cast<const long long *>(st + l.off_first);
    q.cenergy = reinterpret_cast<const double *>(st + l.off_energy); q.amp = reinterpret_cast<const double *>(st + l.off_amp);
    q.head = reinterpret_cast<const MixWsHead *>(ws); q.energy = e.energy; q.plan = reinterpret_cast<int *>(ws + w.off_plan);
    q.user_plan = a.plan; q.plan_words = w.plan_words;
    hipLaunchKernelGGL(mix_plan_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, q);
    err = hipGetLastError();
    if (err != hipSuccess) return err;

    MixPassArgs m{};
    m.in = a.in; m.out = a.out; m.B = a.B; m.S = a.S; m.tiles = (a.S + MIX_TILE - 1) / MIX_TILE; m.nsamp = a.nsamp;
    m.plan = q.plan; m.plan_words = w.plan_words; m.bank = a.bank; m.state = q.state; m.first = q.first;
    m.inplace = f32 && static_cast<const void *>(a.out) == a.in;
    const long long total = (long long)a.B * m.tiles;
    const unsigned blocks = (unsigned)(total < MIX_PASS_BLOCKS ? total : MIX_PASS_BLOCKS);
    if (f32) hipLaunchKernelGGL(mix_pass_kernel<UVAD_INGEST_F32>, dim3(blocks), dim3(MIX_PASS_THREADS), 0, s, m);
    else hipLaunchKernelGGL(mix_pass_kernel<UVAD_INGEST_I16>, dim3(blocks), dim3(MIX_PASS_THREADS), 0, s, m);
    return hipGetLastError();
}

}  // namespace uvad
