// score.hip -- scoring against reference labels (uvad_score_*, uvad_intervals_to_labels, include/uvad.h): what VadModel.test_step logs
// (tp / fp / tn / fn at up to eight operating points, the BCE loss sum) plus a histogram of the raw probabilities per class that gives
// the false-alarm and miss counts at every threshold j / bins, accumulated on the device over any number of batches.
//
// One workgroup per (row, segment of `seg` frames), a one-dimensional grid of B x segments.  It lays the frames [s0 - halo, s1 + halo) of its row out as bit strings in LDS, one
// __ballot word per 64 frames and zeros outside [0, len): X_m = !(p < thr_m) per operating point, G = (gt != 0) and D, the reference
// boundaries (bit k set iff 1 <= k < len and gt[k - 1] != gt[k]).  With rank(i) = ones below bit i (a per-word prefix of popcounts), the
// median label of frame t at point m is rank_m(t + h + 1) - rank_m(t - h) > h and the frame is inside a collar iff
// rank_D(t + c + 1) != rank_D(t - c + 1): two LDS reads and two popcounts each, whatever the kernel size and the collar (the idiom of
// endpoint.hip).  halo = max(h_m, c), so no output depends on where the segments are cut.  A wave scores 64 frames at a time and counts
// with popcounts of ballots; the histogram lives in LDS and only its non-zero bins reach the state.
//   score_reset_kernel    header and a zero record
//   score_step_kernel     the step above: integer totals by vector integer atomics, point 0's counts and the loss of the (row, segment)
//                         as a partial in the workspace
//   score_fold_kernel     the partials in a fixed order: per-row counts, the step's loss sum (workspace head) and the state's double --
//                         no floating-point atomics, so the same calls give the same bits
//   score_totals_kernel   the record, copied out
//   iv_labels_kernel      reference intervals -> label rows: zero fill, barrier, every interval's span stored as plain bytes
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

static_assert(SC_RECORD_WORDS == UVAD_SCORE_TOTALS_WORDS && SC_MAX_POINTS == UVAD_SCORE_MAX_POINTS, "the record of include/uvad.h");
static_assert(sizeof(ScoreHeader) == 256 && sizeof(ScorePartial) == 32 && sizeof(ScoreWsHead) == 32, "state and workspace layout");

namespace {

__device__ __forceinline__ int sc_row_len(const int *lens, int b, int T) {
    if (!lens) return T;
    const int n = lens[b];
    return n < 0 ? 0 : n > T ? T : n;
}

__global__ __launch_bounds__(256) void score_reset_kernel(unsigned *state, int n_points, int bins) {
    const int n = (int)(score_state_bytes() / sizeof(unsigned));
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        unsigned v = 0u;
        if (i == 0) v = SC_MAGIC;
        else if (i == 1) v = (unsigned)n_points;
        else if (i == 2) v = (unsigned)bins;
        else if (i == (int)(sizeof(ScoreHeader) / sizeof(unsigned)) + 2 * SC_W_POINTS) v = (unsigned)n_points;
        else if (i == (int)(sizeof(ScoreHeader) / sizeof(unsigned)) + 2 * SC_W_BINS) v = (unsigned)bins;
        state[i] = v;
    }
}

// NW: the 64-bit words per bit string the launch's LDS holds (frames of a segment and two halos, plus one zero word)
__global__ __launch_bounds__(256) void score_step_kernel(ScoreArgs a, int NW) {
    extern __shared__ unsigned long long sc_words[];
    const ScoreHeader *hd = reinterpret_cast<const ScoreHeader *>(a.state);
    if (hd->magic != SC_MAGIC || hd->n_points != a.n_points || hd->bins != a.bins) return;   // not the state this launch was made for
    unsigned long long *rec = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(a.state) + sizeof(ScoreHeader));
    const int sg = (int)(blockIdx.x % (unsigned)a.nseg), b = (int)(blockIdx.x / (unsigned)a.nseg), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = a.n_points, c = a.collar, bins = a.bins;
    ScorePartial *part = reinterpret_cast<ScorePartial *>(reinterpret_cast<char *>(a.ws) + sizeof(ScoreWsHead)) + (size_t)b * a.nseg + sg;
    const int n = sc_row_len(a.lens, b, a.T);
    const int s0 = sg * a.seg;                                   // < T <= 2^30
    if (s0 >= n) {                                               // nothing of this row here: no read, an empty partial
        if (tid == 0) *part = ScorePartial{0.0, 0u, 0u, 0u, 0u, {0u, 0u}};
        return;
    }
    const int s1 = s0 + a.seg < n ? s0 + a.seg : n;
    const int a0 = s0 - a.halo;                                  // frame of bit 0 (may be negative: those bits are zero)
    const int nw = (s1 - s0 + 2 * a.halo + 63) >> 6;             // words that hold frames; word nw is zero; nw + 1 <= NW
    // LDS: np + 2 strings of NW words (X_0 .. X_{np-1}, D, G) | 4 doubles | np + 1 prefix arrays of NW + 1 ints | 2 * bins | 2 * np + 2 counters
    unsigned long long *Dw = sc_words + (size_t)np * NW, *Gw = Dw + NW;
    double *lossw = reinterpret_cast<double *>(Gw + NW);
    int *pc = reinterpret_cast<int *>(lossw + 4);
    unsigned *hist = reinterpret_cast<unsigned *>(pc + (size_t)(np + 1) * (NW + 1));
    unsigned *cnt = hist + 2 * bins;                             // tp[m] at 2 m, fp[m] at 2 m + 1, then scored speech, scored non-speech
    const float *prow = a.probs + (size_t)b * a.ld_p;
    const uint8_t *grow = a.gt + (size_t)b * a.ld_gt;

    for (int i = tid; i < 2 * bins + 2 * np + 2; i += 256) hist[i] = 0u;
    for (int j = wave; j < nw; j += 4) {
        const int f = a0 + 64 * j + lane;
        const bool in = f >= 0 && f < n;                         // columns at or past len_b are never read
        float p = 0.0f;
        bool g = false;
        if (in) { p = prow[f]; g = grow[f] != 0; }
        for (int m = 0; m < np; ++m) {
            const unsigned long long w = __ballot(in && !(p < a.thr[m]));   // NaN counts as speech, as median_kernel
            if (lane == 0) sc_words[(size_t)m * NW + j] = w;
        }
        const unsigned long long w = __ballot(in && g);
        if (lane == 0) Gw[j] = w;
    }
    if (tid < np + 2) sc_words[(size_t)tid * NW + nw] = 0ull;
    __syncthreads();
    for (int j = tid; j < nw; j += 256) {
        const unsigned long long g = Gw[j], below = j ? Gw[j - 1] >> 63 : 0ull;
        const long long f0 = (long long)a0 + 64ll * j;
        long long lo = 1 - f0, hi = (long long)n - f0;           // bits of frames 1 .. n - 1
        if (lo < 0) lo = 0;
        if (j == 0 && lo < 1) lo = 1;                            // bit 0 of the window has no predecessor here (and is never asked for)
        if (hi > 64) hi = 64;
        unsigned long long mask = 0ull;
        if (lo < hi) mask = (hi == 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
        Dw[j] = (g ^ ((g << 1) | below)) & mask;
    }
    __syncthreads();
    // pc[s][w] = ones of string s in words below w (strings X_0 .. X_{np-1} and D)
    for (int s = wave; s <= np; s += 4) {
        const unsigned long long *ws = sc_words + (size_t)s * NW;
        int *ps = pc + (size_t)s * (NW + 1);
        int carry = 0;
        for (int w0 = 0; w0 <= nw; w0 += 64) {
            const int w = w0 + lane;
            int v = w <= nw ? __popcll(ws[w]) : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(v, o);
                if (lane >= o) v += u;
            }
            if (w <= nw) ps[w + 1] = carry + v;
            carry += __shfl(v, 63);
        }
        if (lane == 0) ps[0] = 0;
    }
    __syncthreads();

    auto rank = [&](int s, int i) {
        return pc[(size_t)s * (NW + 1) + (i >> 6)] + __popcll(sc_words[(size_t)s * NW + (i >> 6)] & ((1ull << (i & 63)) - 1ull));
    };
    unsigned tp[SC_MAX_POINTS], fp[SC_MAX_POINTS], pos = 0u, neg = 0u;
#pragma unroll
    for (int m = 0; m < SC_MAX_POINTS; ++m) tp[m] = fp[m] = 0u;
    double lsum = 0.0;
    const int nchunk = (s1 - s0 + 63) >> 6;
    for (int q = wave; q < nchunk; q += 4) {
        const int t = s0 + 64 * q + lane;
        const bool valid = t < s1;
        const int i = t - a0;                                    // >= halo; i + halo + 1 <= 64 * nw + 63 for every valid frame
        bool g = false, scored = false;
        float p = 0.0f;
        if (valid) {
            p = prow[t];
            g = (Gw[i >> 6] >> (i & 63)) & 1ull;
            scored = c == 0 || rank(np, i + c + 1) == rank(np, i - c + 1);
            const double q1 = g ? (double)p : 1.0 - (double)p;   // exact: p is an f32
            double l = log(q1);                                  // NaN stays NaN (a NaN probability, or one outside [0, 1])
            if (l < -100.0) l = -100.0;                          // F.binary_cross_entropy's clamp; log(0) = -inf gives exactly 100
            lsum -= l;
            if (scored) {
                const float v = p * (float)bins;                 // exact: bins is a power of two
                const int bin = !(v < (float)bins) ? bins - 1 : v > 0.0f ? (int)v : 0;   // NaN and p >= 1 land in the last bin
                atomicAdd(&hist[(g ? bins : 0) + bin], 1u);
            }
        }
        const unsigned long long Sg = __ballot(scored && g), Sn = __ballot(scored && !g);
        pos += __popcll(Sg);
        neg += __popcll(Sn);
#pragma unroll
        for (int m = 0; m < SC_MAX_POINTS; ++m) {
            if (m < np) {
                const int h = a.half[m];
                const bool y = valid && rank(m, i + h + 1) - rank(m, i - h) > h;
                const unsigned long long Y = __ballot(y);
                tp[m] += __popcll(Y & Sg);
                fp[m] += __popcll(Y & Sn);
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) lsum += __shfl_xor(lsum, o);   // a fixed tree: the same bits every run
    if (lane == 0) {
        lossw[wave] = lsum;
#pragma unroll
        for (int m = 0; m < SC_MAX_POINTS; ++m) {
            if (m < np) {
                if (tp[m]) atomicAdd(&cnt[2 * m], tp[m]);
                if (fp[m]) atomicAdd(&cnt[2 * m + 1], fp[m]);
            }
        }
        if (pos) atomicAdd(&cnt[2 * np], pos);
        if (neg) atomicAdd(&cnt[2 * np + 1], neg);
    }
    __syncthreads();
    const unsigned P = cnt[2 * np], N = cnt[2 * np + 1];
    if (tid < 4 * np) {
        const int m = tid >> 2, k = tid & 3;
        const unsigned t1 = cnt[2 * m], f1 = cnt[2 * m + 1];
        const unsigned v = k == 0 ? t1 : k == 1 ? f1 : k == 2 ? N - f1 : P - t1;   // tp, fp, tn, fn
        if (v) atomicAdd(&rec[SC_W_COUNTS + 4 * m + k], (unsigned long long)v);
    }
    for (int i = tid; i < 2 * bins; i += 256) {
        const unsigned v = hist[i];
        if (v) atomicAdd(&rec[SC_W_HIST + (i >= bins ? SC_MAX_BINS + i - bins : i)], (unsigned long long)v);
    }
    if (tid == 0) {
        const unsigned t1 = cnt[0], f1 = cnt[1];
        *part = ScorePartial{((lossw[0] + lossw[1]) + lossw[2]) + lossw[3], t1, f1, N - f1, P - t1, {0u, 0u}};
    }
}

// one workgroup: thread r folds the rows r, r + 256, ... segment by segment, then the 256 sums meet in a fixed tree
__global__ __launch_bounds__(256) void score_fold_kernel(ScoreArgs a) {
    __shared__ double lsh[256];
    __shared__ unsigned long long vsh[256];
    const ScoreHeader *hd = reinterpret_cast<const ScoreHeader *>(a.state);
    if (hd->magic != SC_MAGIC || hd->n_points != a.n_points || hd->bins != a.bins) return;
    unsigned long long *rec = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(a.state) + sizeof(ScoreHeader));
    ScoreWsHead *head = reinterpret_cast<ScoreWsHead *>(a.ws);
    const ScorePartial *parts = reinterpret_cast<const ScorePartial *>(head + 1);
    const int tid = threadIdx.x;
    double l = 0.0;
    unsigned long long valid = 0ull;
    for (int b = tid; b < a.B; b += 256) {
        unsigned long long r[4] = {0ull, 0ull, 0ull, 0ull};
        double lr = 0.0;
        for (int s = 0; s < a.nseg; ++s) {
            const ScorePartial p = parts[(size_t)b * a.nseg + s];
            lr += p.loss;
            r[0] += p.tp; r[1] += p.fp; r[2] += p.tn; r[3] += p.fn;
        }
        l += lr;
        valid += (unsigned long long)sc_row_len(a.lens, b, a.T);
        if (a.rows)
            for (int k = 0; k < 4; ++k) a.rows[(size_t)b * 4 + k] = r[k];
    }
    lsh[tid] = l;
    vsh[tid] = valid;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) { lsh[tid] += lsh[tid + o]; vsh[tid] += vsh[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        head->loss = lsh[0];
        head->valid = vsh[0];
        rec[SC_W_VALID] += vsh[0];
        rec[SC_W_STEPS] += 1ull;
        double *tot = reinterpret_cast<double *>(rec + SC_W_LOSS);
        *tot += lsh[0];
    }
}

__global__ __launch_bounds__(256) void score_totals_kernel(const unsigned long long *state, unsigned long long *out) {
    const ScoreHeader *hd = reinterpret_cast<const ScoreHeader *>(state);
    const bool ok = hd->magic == SC_MAGIC;
    const unsigned long long *rec = state + sizeof(ScoreHeader) / sizeof(unsigned long long);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < SC_RECORD_WORDS; i += gridDim.x * blockDim.x) out[i] = ok ? rec[i] : 0ull;
}

// one workgroup per (row, column segment); every byte of [0, len_b) in the segment is zeroed, then set by every interval that covers it
constexpr int IVL_SEG = 8192;
__global__ __launch_bounds__(256) void iv_labels_kernel(const int *iv, const int *iv_counts, int max_iv, int T, int ld, const int *lens,
                                                        uint8_t *labels, int nseg) {
    const int b = (int)(blockIdx.x / (unsigned)nseg), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = sc_row_len(lens, b, T);
    const int c0 = (int)(blockIdx.x % (unsigned)nseg) * IVL_SEG;
    if (c0 >= n) return;                                         // columns at or past len_b are not written
    const int c1 = c0 + IVL_SEG < n ? c0 + IVL_SEG : n;
    uint8_t *row = labels + (size_t)b * ld;
    for (int t = c0 + tid; t < c1; t += 256) row[t] = 0;
    __threadfence();
    __syncthreads();                                             // the zeros are in memory before any one is stored over them
    int cnt = iv_counts[b];
    cnt = cnt < 0 ? 0 : cnt > max_iv ? max_iv : cnt;
    const int *mine = iv + (size_t)b * max_iv * 2;
    for (int k = wave; k < cnt; k += 4) {                        // concurrent stores of the same value are fine
        int s = mine[2 * k], e = mine[2 * k + 1];
        s = s < c0 ? c0 : s;
        e = e > c1 ? c1 : e;
        if (s < e)                                               // empty and reversed intervals store nothing (and s + lane cannot wrap)
            for (int t = s + lane; t < e; t += 64) row[t] = 1;
    }
}

}  // namespace

hipError_t launch_score_reset(void *state, int n_points, int bins, hipStream_t s) {
    if (!state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_reset_kernel, dim3(8), dim3(256), 0, s, reinterpret_cast<unsigned *>(state), n_points, bins);
    return hipGetLastError();
}

hipError_t launch_score_step(const ScoreArgs &a, hipStream_t s) {
    if (!a.probs || !a.gt || !a.state || !a.ws || a.B <= 0 || a.T <= 0 || a.T > SC_MAX_T || a.n_points < 1 || a.n_points > SC_MAX_POINTS ||
        a.seg < 1 || a.seg > SC_MAX_SEGMENT || a.halo < 0 || a.halo > SC_MAX_COLLAR || a.bins < 2 || a.bins > SC_MAX_BINS || a.nseg != score_nseg(a.T, a.seg) ||
        (long long)a.B * a.nseg > 0x7fffffffll)
        return hipErrorInvalidValue;
    const int NW = ((a.seg + 2 * a.halo + 63) >> 6) + 1;
    const size_t lds = (size_t)(a.n_points + 2) * NW * sizeof(unsigned long long) + 4 * sizeof(double) +
                       (size_t)(a.n_points + 1) * (NW + 1) * sizeof(int) + (size_t)(2 * a.bins + 2 * a.n_points + 2) * sizeof(unsigned);
    hipLaunchKernelGGL(score_step_kernel, dim3((unsigned)(a.B * a.nseg)), dim3(256), lds, s, a, NW);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(score_fold_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_score_totals(const void *state, unsigned long long *out, hipStream_t s) {
    if (!state || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_totals_kernel, dim3(4), dim3(256), 0, s, reinterpret_cast<const unsigned long long *>(state), out);
    return hipGetLastError();
}

hipError_t launch_intervals_to_labels(const int *iv, const int *iv_counts, int B, int max_iv, int T, int ld, const int *lens, uint8_t *labels,
                                      hipStream_t s) {
    if (!iv_counts || !labels || B <= 0 || T <= 0 || T > SC_MAX_T || ld < T || max_iv < 0 || (max_iv > 0 && !iv)) return hipErrorInvalidValue;
    const int nseg = (T + IVL_SEG - 1) / IVL_SEG;
    if ((long long)B * nseg > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(iv_labels_kernel, dim3((unsigned)(B * nseg)), dim3(256), 0, s, iv, iv_counts, max_iv, T, ld, lens, labels, nseg);
    return hipGetLastError();
}

}  // namespace uvad
