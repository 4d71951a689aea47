// sampler.hip -- training batches drawn on the device (uvad_sampler_*, include/uvad.h): the corpus stays on the device as recordings back to
// back; a step plans B rows (dataset by weight, position in the dataset's shuffled epoch, window), gathers their samples and rasterises their
// frame labels.  What the reference does on the host with cut_into_windows / filter / pad, SimpleCutSampler, CutSet.mux and
// supervisions_feature_mask.  A step is three launches:
//   sampler_plan_kernel        ONE workgroup.  Its first thread takes the draw ordinal, threads d < D the cursors, from the state
//                              (uvad_sampler_step, advancing them at the end) or from the caller (uvad_sampler_apply).  A thread per row draws
//                              the row's dataset; thread d then walks the rows in order and numbers those of dataset d (the row's rank among
//                              its dataset's rows: no atomics, the order is the row order); a thread per row turns (cursor + rank) into
//                              (epoch, position), the position into a window by the Feistel walk of include/uvad.h (never a stored
//                              permutation), the window into (recording, start, n) by a binary search over the slots' first windows, and
//                              writes the plan row to the workspace, and to d_plan when that is given.
//   sampler_gather_kernel<fmt> one workgroup per (row, 4096 output samples): 16-byte stores from the output row's first 16-byte boundary;
//                              16-byte (f32) / 8-byte (int16) loads when the source is aligned with them, loads of 4- / 2-byte alignment
//                              otherwise; the samples in front of the boundary and behind the last whole group element by element; +0 from n to W.
//   sampler_label_kernel       one workgroup per row: d_nsamp and d_frames, a zero fill of the row's T bytes, a barrier, then the threads stride
//                              over the recording's supervisions and store ones (every writer of a byte stores the same value).
// sampler_build is the host side of uvad_sampler_reset: it validates the tables and builds the state's image; tests/sampler_ref.py restates all of it.
#include "../../include/uvad.h"
#include "philox.h"
#include "uvad_internal.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace uvad {

static_assert(sizeof(SamplerHeader) == 256 && sizeof(SamplerSet) == 32, "state layout");
static_assert(offsetof(SamplerHeader, W) == 16 && offsetof(SamplerHeader, seed) == 24 && offsetof(SamplerHeader, total) == 32 &&
              offsetof(SamplerHeader, fmt) == 40 && offsetof(SamplerHeader, n_windows) == 48 && offsetof(SamplerHeader, draws) == 56 &&
              offsetof(SamplerHeader, shuffle) == 64 && offsetof(SamplerHeader, step) == 80 && offsetof(SamplerHeader, kw) == 96 &&
              offsetof(SamplerHeader, min_keep) == 112, "the header of include/uvad.h");
static_assert(SAMPLER_PLAN_WORDS == UVAD_SAMPLER_PLAN_WORDS && SAMPLER_MAX_SETS == UVAD_SAMPLER_MAX_SETS, "the constants of include/uvad.h");

static size_t sampler_pad(size_t v) { return (v + 255) / 256 * 256; }

SamplerLayout sampler_layout(int R, int n_sup) {
    SamplerLayout l{};
    l.off_sets = sizeof(SamplerHeader);
    l.off_slot = l.off_sets + sampler_pad(sizeof(SamplerSet) * SAMPLER_MAX_SETS);
    l.off_win = l.off_slot + sampler_pad((size_t)R * 4);
    l.off_first = l.off_win + sampler_pad(((size_t)R + 1) * 4);
    l.off_supf = l.off_first + sampler_pad(((size_t)R + 1) * 8);
    l.off_sup = l.off_supf + sampler_pad(((size_t)R + 1) * 4);
    l.total = l.off_sup + sampler_pad((size_t)n_sup * 16);
    return l;
}

size_t sampler_ws_bytes(int B) { return sizeof(MixWsHead) + sampler_pad((size_t)B * SAMPLER_PLAN_WORDS * 4); }

const char *sampler_build(const SamplerTables &t, char *image) {
    const uvad_sampler_cfg &q = *t.q;
    const int R = t.R, D = t.D;
    const long long W = q.window, keep = q.min_keep;
    if (t.rec_first[0] != 0) return "h_rec_first[0] must be 0";
    for (int r = 0; r < R; ++r) {
        const long long len = t.rec_first[r + 1] - t.rec_first[r];
        if (len <= 0) return "h_rec_first must increase: an empty recording";
        if (len > SAMPLER_MAX_LEN) return "a recording has more than 2^31 - 1 samples";
    }
    if (t.sup_first[0] != 0 || t.sup_first[R] != t.n_sup) return "h_sup_first must run from 0 to n_sup";
    for (int r = 0; r < R; ++r)
        if (t.sup_first[r + 1] < t.sup_first[r]) return "h_sup_first must not decrease";
    for (int r = 0; r < R; ++r)
        if (t.rec_set[r] < 0 || t.rec_set[r] >= D) return "h_rec_set: a dataset index out of range";
    double sum = 0.0;
    for (int d = 0; d < D; ++d) {
        if (!std::isfinite(t.weight[d]) || !(t.weight[d] > 0.0)) return "h_weight: a weight must be finite and > 0";
        sum += t.weight[d];
    }
    if (!std::isfinite(sum)) return "h_weight: the weights' sum must be finite";

    const SamplerLayout l = sampler_layout(R, t.n_sup);
    SamplerHeader *h = reinterpret_cast<SamplerHeader *>(image);
    SamplerSet *sets = reinterpret_cast<SamplerSet *>(image + l.off_sets);
    int *slot = reinterpret_cast<int *>(image + l.off_slot), *win = reinterpret_cast<int *>(image + l.off_win);
    long long n_all = 0;
    int j = 0;
    for (int d = 0; d < D; ++d) {                              // grouped by dataset, recording order inside a dataset
        const long long first = n_all;
        for (int r = 0; r < R; ++r) {
            if (t.rec_set[r] != d) continue;
            const long long len = t.rec_first[r + 1] - t.rec_first[r], full = len / W, rest = len - full * W;
            slot[j] = r; win[j] = (int)n_all; ++j;
            n_all += full + (rest > keep ? 1 : 0);             // strict: a tail of exactly min_keep samples goes
            if (n_all > SAMPLER_MAX_LEN) return "more than 2^31 - 1 windows";
        }
        if (n_all == first) return "a dataset without windows";
        sets[d].cursor = 0; sets[d].first = (int)first; sets[d].N = (int)(n_all - first); sets[d].L = n_all - first;
    }
    win[R] = (int)n_all;
    if (q.drop_last) {
        if (sets[0].N < q.batch) return "drop_last: fewer windows than batch";
        sets[0].L = (long long)(sets[0].N / q.batch) * q.batch;
    }
    double part = 0.0;
    for (int d = 0; d < D; ++d) {
        part += t.weight[d];
        sets[d].cum = (unsigned long long)std::floor(part / sum * 4294967296.0);
    }
    sets[D - 1].cum = 4294967296ULL;
    h->magic = SAMPLER_MAGIC; h->R = R; h->n_sup = t.n_sup; h->D = D; h->W = W; h->seed = q.seed; h->total = t.rec_first[R]; h->fmt = t.fmt;
    h->geometry = q.geometry; h->n_windows = (int)n_all; h->batch = q.batch; h->draws = 0; h->shuffle = q.shuffle != 0;
    h->drop_last = q.drop_last != 0; h->pad = q.pad != 0; h->half = q.half; h->step = q.step; h->min_keep = keep;
    std::memcpy(image + l.off_first, t.rec_first, ((size_t)R + 1) * 8);
    std::memcpy(image + l.off_supf, t.sup_first, ((size_t)R + 1) * 4);
    if (t.n_sup > 0) std::memcpy(image + l.off_sup, t.sup, (size_t)t.n_sup * 16);
    return nullptr;
}

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_TILE_GROUPS = 1024;                            // 16-byte groups of one gather workgroup: 4 per thread, 4096 samples

typedef float sp_f4 __attribute__((ext_vector_type(4)));
typedef short sp_s4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) sp_f4u { float v[4]; };   // a group whose source is only element-aligned
struct __attribute__((packed, aligned(2))) sp_s4u { short v[4]; };

// the epoch order of include/uvad.h: position p of epoch e of dataset d -> a window index below N
__device__ __forceinline__ unsigned sp_perm(unsigned N, unsigned long long seed, unsigned d, unsigned long long e, unsigned p, int shuffle) {
    if (!shuffle || N <= 1) return p;
    int k = 32 - __clz((int)(N - 1));
    k = k < 8 ? 8 : k;
    k += k & 1;
    const int half = k >> 1;
    const unsigned mask = (1u << half) - 1;
    unsigned long long x = p;
    do {
        unsigned L = (unsigned)(x >> half), R = (unsigned)x & mask;
#pragma unroll
        for (unsigned t = 0; t < 4; ++t) {
            const uint4 w = lt_philox(make_uint4(R | (t << 16), 0x53500000u | d, (unsigned)e, (unsigned)(e >> 32)), (unsigned)seed, (unsigned)(seed >> 32));
            const unsigned nr = L ^ (w.x & mask);
            L = R; R = nr;
        }
        x = ((unsigned long long)L << half) | R;
    } while (x >= N);
    return (unsigned)x;
}

struct SamplerPlanArgs {
    int B; SamplerHeader *state; SamplerSet *sets; const int *slot; const int *win; const long long *rec_first; MixWsHead *head; int *plan; int *user_plan;
    int take; unsigned long long draw; long long row0; long long cursor[SAMPLER_MAX_SETS];
};

__global__ __launch_bounds__(SP_THREADS) void sampler_plan_kernel(SamplerPlanArgs a) {
    __shared__ unsigned s_draw[2];
    __shared__ long long s_cur[SAMPLER_MAX_SETS];
    __shared__ int s_cnt[SAMPLER_MAX_SETS];
    const int tid = threadIdx.x;
    const SamplerHeader &hd = *a.state;
    const bool ok = hd.magic == SAMPLER_MAGIC && hd.D >= 1 && hd.D <= SAMPLER_MAX_SETS && hd.R >= 1;
    const int D = ok ? hd.D : 0;                                // (a state that lost its magic plans rows of no samples: nothing is read)
    if (tid == 0) {
        const unsigned long long d = a.take ? hd.draws : a.draw;
        a.head->draw = d; a.head->row0 = a.row0;
        s_draw[0] = (unsigned)d; s_draw[1] = (unsigned)(d >> 32);
    }
    if (tid < SAMPLER_MAX_SETS) {
        s_cur[tid] = tid < D ? (a.take ? a.sets[tid].cursor : a.cursor[tid]) : 0;
        s_cnt[tid] = 0;
    }
    __syncthreads();
    const unsigned long long seed = hd.seed;
    for (int b = tid; b < a.B; b += SP_THREADS) {               // the row's dataset, kept in word 0 of its plan row
        const uint4 w = lt_philox(make_uint4((unsigned)(a.row0 + b), 0x53440000u, s_draw[0], s_draw[1]), (unsigned)seed, (unsigned)(seed >> 32));
        int d = 0;
        while (d < D - 1 && (unsigned long long)w.x >= a.sets[d].cum) ++d;
        a.plan[(size_t)b * SAMPLER_PLAN_WORDS] = d;
    }
    __syncthreads();
    if (tid < D) {                                              // the rank of every row among its dataset's rows, in row order (word 2, for now)
        int n = 0;
        for (int b = 0; b < a.B; ++b)
            if (a.plan[(size_t)b * SAMPLER_PLAN_WORDS] == tid) a.plan[(size_t)b * SAMPLER_PLAN_WORDS + 2] = n++;
        s_cnt[tid] = n;
    }
    __syncthreads();
    for (int b = tid; b < a.B; b += SP_THREADS) {
        int *p = a.plan + (size_t)b * SAMPLER_PLAN_WORDS;
        int rec[SAMPLER_PLAN_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ok) {
            const int d = p[0];
            const SamplerSet st = a.sets[d];
            const unsigned long long c = (unsigned long long)(s_cur[d] + p[2]), L = (unsigned long long)st.L;
            const unsigned long long e = c / L;
            const unsigned pos = (unsigned)(c - e * L);
            const int w = st.first + (int)sp_perm((unsigned)st.N, seed, (unsigned)d, e, pos, hd.shuffle);
            int lo = 0, hi = hd.R;                              // the last slot whose first window is <= w: win[lo] <= w < win[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (a.win[mid] <= w) lo = mid; else hi = mid;
            }
            const int r = a.slot[lo];
            const long long len = a.rec_first[r + 1] - a.rec_first[r], start = (long long)(w - a.win[lo]) * hd.W;
            const long long n = len - start < hd.W ? len - start : hd.W;
            rec[0] = d; rec[1] = (int)(unsigned)e; rec[2] = (int)pos; rec[3] = w; rec[4] = r; rec[5] = (int)start; rec[6] = (int)n;
            rec[7] = (int)sampler_frames(hd, hd.pad ? hd.W : n);
        }
#pragma unroll
        for (int i = 0; i < SAMPLER_PLAN_WORDS; ++i) p[i] = rec[i];
        if (a.user_plan) {
#pragma unroll
            for (int i = 0; i < SAMPLER_PLAN_WORDS; ++i) a.user_plan[(size_t)b * SAMPLER_PLAN_WORDS + i] = rec[i];
        }
    }
    if (a.take && tid < D) a.sets[tid].cursor = s_cur[tid] + s_cnt[tid];     // s_cur / s_cnt: read-only since the last barrier
    if (a.take && tid == 0) a.state->draws = ((unsigned long long)s_draw[1] << 32 | s_draw[0]) + 1;
}

struct SamplerGatherArgs { const void *pcm; const long long *rec_first; const int *plan; float *out; long long ld_out, W; int tiles; };

template <int FMT>
__device__ __forceinline__ float sp_load(const void *src, long long i) {
    if constexpr (FMT == UVAD_INGEST_F32) return reinterpret_cast<const float *>(src)[i];
    else return (float)reinterpret_cast<const short *>(src)[i] * (1.0f / 32768.0f);
}

template <int FMT>
__global__ __launch_bounds__(SP_THREADS) void sampler_gather_kernel(SamplerGatherArgs a) {
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / a.tiles;
    const int tile = (int)(blockIdx.x - b * a.tiles);
    const int *p = a.plan + (size_t)b * SAMPLER_PLAN_WORDS;
    const long long n = p[6], W = a.W;                          // n <= W; n = 0 (a lost state): the row is zeros and `src` is never read
    const long long s0 = a.rec_first[p[4]] + p[5];
    const void *src = FMT == UVAD_INGEST_F32 ? static_cast<const void *>(reinterpret_cast<const float *>(a.pcm) + s0)
                                             : static_cast<const void *>(reinterpret_cast<const short *>(a.pcm) + s0);
    float *drow = a.out + b * a.ld_out;
    long long head = (long long)(((16 - (reinterpret_cast<uintptr_t>(drow) & 15)) & 15) >> 2);   // samples in front of the row's first 16-byte boundary
    head = head < W ? head : W;
    const long long groups = (W - head) >> 2, tail0 = head + 4 * groups;
    if (tile == 0) {                                            // at most 3 samples in front, at most 3 behind
        long long i = -1;
        if (tid < head) i = tid;
        else if (tid >= 4 && tail0 + (tid - 4) < W && tid < 8) i = tail0 + (tid - 4);
        if (i >= 0) drow[i] = i < n ? sp_load<FMT>(src, i) : 0.0f;
    }
    constexpr int ELEM = FMT == UVAD_INGEST_F32 ? 4 : 2;
    const bool aligned = ((reinterpret_cast<uintptr_t>(src) + (uintptr_t)head * ELEM) & (4 * ELEM - 1)) == 0;   // block-uniform
#pragma unroll
    for (int u = 0; u < SP_TILE_GROUPS / SP_THREADS; ++u) {
        const long long g = (long long)tile * SP_TILE_GROUPS + u * SP_THREADS + tid;
        if (g >= groups) continue;
        const long long i = head + 4 * g;
        sp_f4 v;
        if (i + 4 <= n) {
            if constexpr (FMT == UVAD_INGEST_F32) {
                const float *s = reinterpret_cast<const float *>(src) + i;
                if (aligned) v = *reinterpret_cast<const sp_f4 *>(s);
                else { const sp_f4u q = *reinterpret_cast<const sp_f4u *>(s); v = sp_f4{q.v[0], q.v[1], q.v[2], q.v[3]}; }
            } else {
                const short *s = reinterpret_cast<const short *>(src) + i;
                short q0, q1, q2, q3;
                if (aligned) { const sp_s4 q = *reinterpret_cast<const sp_s4 *>(s); q0 = q.x; q1 = q.y; q2 = q.z; q3 = q.w; }
                else { const sp_s4u q = *reinterpret_cast<const sp_s4u *>(s); q0 = q.v[0]; q1 = q.v[1]; q2 = q.v[2]; q3 = q.v[3]; }
                v = sp_f4{(float)q0 * (1.0f / 32768.0f), (float)q1 * (1.0f / 32768.0f), (float)q2 * (1.0f / 32768.0f), (float)q3 * (1.0f / 32768.0f)};
            }
        } else {                                                // the group that holds sample n, and the zeros behind it
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = i + e < n ? sp_load<FMT>(src, i + e) : 0.0f;
        }
        *reinterpret_cast<sp_f4 *>(drow + i) = v;
    }
}

struct SamplerLabelArgs {
    const SamplerHeader *state; const int *sup_first; const long long *sup; const int *plan;
    long long *nsamp; unsigned char *labels; long long ld_gt; int *frames; long long T;
};

__device__ __forceinline__ long long sp_floordiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0

__global__ __launch_bounds__(SP_THREADS) void sampler_label_kernel(SamplerLabelArgs a) {
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const SamplerHeader &hd = *a.state;
    const int *p = a.plan + (size_t)b * SAMPLER_PLAN_WORDS;
    const long long start = p[5], n = p[6], Tb = p[7] < a.T ? p[7] : a.T;
    const long long len = hd.pad ? hd.W : n;
    unsigned char *row = a.labels + b * a.ld_gt;
    if (tid == 0) { a.nsamp[b] = len; a.frames[b] = (int)Tb; }
    for (long long t = tid; t < a.T; t += SP_THREADS) row[t] = 0;
    __syncthreads();                                            // the zeros are stored before any one
    if (n <= 0) return;
    const int r = p[4];
    for (int s = a.sup_first[r] + tid; s < a.sup_first[r + 1]; s += SP_THREADS) {
        long long ss = a.sup[2 * (size_t)s], se = a.sup[2 * (size_t)s + 1];
        ss = ss < 0 ? 0 : ss; se = se < 0 ? 0 : se;             // (a negative bound clips to the window's edge anyway; no overflow below)
        const long long rs = ss - start > 0 ? ss - start : 0, re = se - start < n ? se - start : n;
        if (re <= rs) continue;
        long long st, et;
        if (hd.geometry == UVAD_SAMPLER_FBANK) {
            st = rs / hd.hop; et = re / hd.hop;
        } else {
            st = rs > 0 ? sp_floordiv(rs - hd.half, hd.step) : 0;
            et = re < len ? sp_floordiv(re - hd.half, hd.step) : Tb;
            st = st > 0 ? st : 0; et = et > 0 ? et : 0;
        }
        et = et < Tb ? et : Tb;
        for (long long t = st; t < et; ++t) row[t] = 1;
    }
}

__global__ __launch_bounds__(SAMPLER_MAX_SETS) void sampler_read_kernel(const SamplerHeader *h, const SamplerSet *sets, int D, long long *out) {
    const int t = threadIdx.x;
    if (t == 0) out[0] = (long long)h->draws;
    if (t < D) out[1 + t] = sets[t].cursor;
}

__global__ __launch_bounds__(SAMPLER_MAX_SETS) void sampler_write_kernel(SamplerHeader *h, SamplerSet *sets, int D, const long long *in) {
    const int t = threadIdx.x;
    if (t == 0) h->draws = (unsigned long long)in[0];
    if (t < D) sets[t].cursor = in[1 + t] < 0 ? 0 : in[1 + t];  // positions are counts
}

}  // namespace

hipError_t launch_sampler(const SamplerArgs &a, hipStream_t s) {
    if (!a.out || !a.nsamp || !a.labels || !a.frames || !a.pcm || !a.state || !a.ws || a.B < 1 || a.R < 1 || a.n_sup < 0 || a.D < 1 ||
        a.D > SAMPLER_MAX_SETS || a.W < 1 || a.W > SAMPLER_MAX_LEN || a.T < 1 || a.ld_out < a.W || a.ld_gt < a.T ||
        (a.fmt != UVAD_INGEST_F32 && a.fmt != UVAD_INGEST_I16))
        return hipErrorInvalidValue;
    const long long tiles = (a.W / 4 + SP_TILE_GROUPS - 1) / SP_TILE_GROUPS > 0 ? (a.W / 4 + SP_TILE_GROUPS - 1) / SP_TILE_GROUPS : 1;
    if ((long long)a.B * tiles > 2147483647LL) return hipErrorInvalidValue;
    const SamplerLayout l = sampler_layout(a.R, a.n_sup);
    char *st = reinterpret_cast<char *>(a.state), *ws = reinterpret_cast<char *>(a.ws);
    int *plan = reinterpret_cast<int *>(ws + sizeof(MixWsHead));
    const long long *rec_first = reinterpret_cast<const long long *>(st + l.off_first);

    SamplerPlanArgs q{};
    q.B = a.B; q.state = reinterpret_cast<SamplerHeader *>(st); q.sets = reinterpret_cast<SamplerSet *>(st + l.off_sets);
    q.slot = reinterpret_cast<const int *>(st + l.off_slot); q.win = reinterpret_cast<const int *>(st + l.off_win); q.rec_first = rec_first;
    q.head = reinterpret_cast<MixWsHead *>(ws); q.plan = plan; q.user_plan = a.plan; q.take = a.take ? 1 : 0; q.draw = a.draw; q.row0 = a.row0;
    for (int d = 0; d < SAMPLER_MAX_SETS; ++d) q.cursor[d] = d < a.D ? a.cursor[d] : 0;
    hipLaunchKernelGGL(sampler_plan_kernel, dim3(1), dim3(SP_THREADS), 0, s, q);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;

    SamplerGatherArgs g{};
    g.pcm = a.pcm; g.rec_first = rec_first; g.plan = plan; g.out = a.out; g.ld_out = a.ld_out; g.W = a.W; g.tiles = (int)tiles;
    const unsigned blocks = (unsigned)((long long)a.B * tiles);
    if (a.fmt == UVAD_INGEST_F32) hipLaunchKernelGGL(sampler_gather_kernel<UVAD_INGEST_F32>, dim3(blocks), dim3(SP_THREADS), 0, s, g);
    else hipLaunchKernelGGL(sampler_gather_kernel<UVAD_INGEST_I16>, dim3(blocks), dim3(SP_THREADS), 0, s, g);
    err = hipGetLastError();
    if (err != hipSuccess) return err;

    SamplerLabelArgs k{};
    k.state = reinterpret_cast<const SamplerHeader *>(st); k.sup_first = reinterpret_cast<const int *>(st + l.off_supf);
    k.sup = reinterpret_cast<const long long *>(st + l.off_sup); k.plan = plan; k.nsamp = a.nsamp; k.labels = a.labels; k.ld_gt = a.ld_gt;
    k.frames = a.frames; k.T = a.T;
    hipLaunchKernelGGL(sampler_label_kernel, dim3((unsigned)a.B), dim3(SP_THREADS), 0, s, k);
    return hipGetLastError();
}

hipError_t launch_sampler_read(const void *state, int D, long long *out, hipStream_t s) {
    if (!state || !out || D < 1 || D > SAMPLER_MAX_SETS) return hipErrorInvalidValue;
    const char *st = reinterpret_cast<const char *>(state);
    hipLaunchKernelGGL(sampler_read_kernel, dim3(1), dim3(SAMPLER_MAX_SETS), 0, s, reinterpret_cast<const SamplerHeader *>(st),
                       reinterpret_cast<const SamplerSet *>(st + sizeof(SamplerHeader)), D, out);
    return hipGetLastError();
}

hipError_t launch_sampler_write(void *state, int D, const long long *in, hipStream_t s) {
    if (!state || !in || D < 1 || D > SAMPLER_MAX_SETS) return hipErrorInvalidValue;
    char *st = reinterpret_cast<char *>(state);
    hipLaunchKernelGGL(sampler_write_kernel, dim3(1), dim3(SAMPLER_MAX_SETS), 0, s, reinterpret_cast<SamplerHeader *>(st),
                       reinterpret_cast<SamplerSet *>(st + sizeof(SamplerHeader)), D, in);
    return hipGetLastError();
}

}  // namespace uvad
