// binarize.hip -- hysteresis decisions with minimum durations on the device (uvad_binarize, include/uvad.h): probabilities -> speech
// intervals and labels by two thresholds (on at !(p < onset), off at p < offset, unchanged in between), asymmetric padding, a shortest
// pause that is filled and a shortest interval that is kept.  Everything after the two comparisons is integer, no atomics: the same
// calls give the same bytes.
//
// The state recurrence s[t] = HI[t] | (MID[t] & s[t - 1]) is the carry chain of a binary addition: with a = HI | MID and b = HI, bit t
// generates a carry where HI, propagates one where MID and kills it where LO, so the carry OUT of bit t of a + b + c is s[t] (c: the
// state below bit 0).  With C = (a + b + c) ^ a ^ b, the carries INTO every bit, the states of a 64-frame word are HI | (MID & C): one
// addition per word.  A word as a whole generates (its top state is 1 with c = 0) or propagates (all 64 frames MID), so the carries
// into the 64 words of a pass are the same addition once more, on the two __ballot masks of those summaries.
//
// After that the row is a row of 0/1 labels and the rest is cuts.hip's walk with 2 P replaced by D = pad_on + pad_off + max(min_off -
// 1, 0): runs [s, c) and [s', c') end in one interval iff s' - c <= D.  (Padded, the second starts at max(s' - pad_on, 0) and the first
// ends at min(c + pad_off, n); they merge iff that gap is <= 0 or < min_off, i.e. iff s' - pad_on - c - pad_off < max(min_off, 1).  A
// start clipped at 0 or an end clipped at n makes the gap <= 0 and the unclipped difference negative: the clipping never changes the
// outcome.)  A run start is REAL iff it is the row's first or its gap is longer than D; a real start (or the row's end) closes the
// interval its predecessor opened, [max(s - pad_on, 0), min(c + pad_off, n)) with c one past the last 1 before it, kept iff it has at
// least min_on frames.
//   binarize_classify_kernel  one workgroup per (row, segment of BIN_SEG frames): 16-byte loads of the probabilities (4-byte loads for
//                             rows that are not 16-byte aligned), two words per 64 frames -- the HI mask and the LO mask, frames at or
//                             past len_b marked LO so that nothing extends past the row -- into the workspace.  Reads 4 B and writes
//                             0.25 B per frame; this is the only frame-proportional work on the probabilities.
//   binarize_rows_kernel      one wave per row, passes of BIN_SPAN_WORDS word pairs, one pair per lane, the next pass's pair in flight
//                             while this one is worked on.  States by the two additions above; then run starts by bit operations, the
//                             last 1 below each by count-leading-zeros, the two prefix maxima and the output positions by wave scans,
//                             as cuts_rows_kernel.  What a pass leaves to the next: the state bit and three integers.  Out: the row's
//                             full interval list in the workspace, its first max_iv entries in d_iv, the true count in d_iv_counts.
//   labels                    the workspace list (never the truncated d_iv) through score.hip's iv_labels_kernel.
#include <cstddef>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

static_assert(sizeof(uvad_binarize_cfg) == 24 && sizeof(BinCfgInt) == 24 && offsetof(uvad_binarize_cfg, min_on) == offsetof(BinCfgInt, min_on) &&
              offsetof(uvad_binarize_cfg, pad_off) == offsetof(BinCfgInt, pad_off), "uvad_binarize_cfg");
static_assert(BIN_MAX_T == (1 << 30) && BIN_SPAN_WORDS == 64 && BIN_SEG == 2048, "frame arithmetic in int32; one word pair per lane; 8 words per classify wave");

namespace {

__device__ __forceinline__ int bin_incl_max(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v = u > v ? u : v;
    }
    return v;
}

__device__ __forceinline__ int bin_incl_sum(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

__device__ __forceinline__ int bin_row_len(const int *lens, int b, int T) {
    if (!lens) return T;
    const int n = lens[b];
    return n < 0 ? 0 : n > T ? T : n;
}

// bit i of the low 16 bits -> bit 4 i
__device__ __forceinline__ unsigned long long bin_spread4(unsigned long long x) {
    x &= 0xffffull;
    x = (x | (x << 24)) & 0x000000ff000000ffull;
    x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

// VEC: every row starts on a 16-byte boundary.  A wave takes BIN_SEG / 4 = 512 frames, 8 words.
template <bool VEC> __global__ __launch_bounds__(256) void binarize_classify_kernel(BinarizeArgs a, int nseg) {
    const int b = (int)(blockIdx.x / (unsigned)nseg), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = bin_row_len(a.lens, b, a.T);
    const int fw = (int)(blockIdx.x % (unsigned)nseg) * BIN_SEG + wave * (BIN_SEG / 4);   // < 2^30 + BIN_SEG
    if (fw >= n) return;                                         // columns at or past len_b are never read; their words are never used
    const float *row = a.probs + (size_t)b * a.ld_p;
    ulonglong2 *out = reinterpret_cast<ulonglong2 *>(a.words) + (size_t)b * a.nwt;
    const int nw = (n + 63) >> 6;                                // <= nwt
    const float on = a.q.onset, off = a.q.offset;
    if (VEC) {
        float4 v[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {                         // both loads first, then the ballots
            const int f = fw + 256 * it + 4 * lane;
            if (f + 3 < n) v[it] = *reinterpret_cast<const float4 *>(row + f);
            else {
                v[it].x = f < n ? row[f] : 0.0f;
                v[it].y = f + 1 < n ? row[f + 1] : 0.0f;
                v[it].z = f + 2 < n ? row[f + 2] : 0.0f;
                v[it].w = 0.0f;                                  // f + 3 >= n here
            }
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int f = fw + 256 * it + 4 * lane;
            const float e[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
            unsigned long long bh[4], bl[4];                     // bit l of mask k: frame 4 l + k of these 256
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool valid = f + k < n;
                bh[k] = __ballot(valid && !(e[k] < on));
                bl[k] = __ballot(!valid || e[k] < off);
            }
            const int w = ((fw + 256 * it) >> 6) + lane;         // lanes 0 .. 3 put one word together each: lanes 16 j .. 16 j + 15
            if (lane < 4 && w < nw) {
                unsigned long long h = 0, l = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    h |= bin_spread4(bh[k] >> (16 * lane)) << k;
                    l |= bin_spread4(bl[k] >> (16 * lane)) << k;
                }
                out[w] = make_ulonglong2(h, l);
            }
        }
    } else {
        constexpr int PER = BIN_SEG / 4 / 64;
        float v[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int f = fw + 64 * k + lane;
            v[k] = f < n ? row[f] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const bool valid = fw + 64 * k + lane < n;
            const unsigned long long h = __ballot(valid && !(v[k] < on)), l = __ballot(!valid || v[k] < off);
            const int w = (fw >> 6) + k;
            if (lane == 0 && w < nw) out[w] = make_ulonglong2(h, l);
        }
    }
}

// the real starts among the run starts `rise` of the word x (frames f0 .. f0 + 63), in ascending order: f(s, c) with c one past the last 1
// before s (0: the row's first run); `before` is that for the words below this one
template <class F> __device__ __forceinline__ void bin_walk(unsigned long long x, unsigned long long rise, int f0, int before, int D, F &&f) {
    while (rise) {
        const int i = __builtin_ctzll(rise);
        rise &= rise - 1ull;
        const unsigned long long below = x & ((1ull << i) - 1ull);
        const int c = below ? f0 + 64 - __clzll((long long)below) : before;
        if (c == 0 || f0 + i - c > D) f(f0 + i, c);
    }
}

__global__ __launch_bounds__(64) void binarize_rows_kernel(BinarizeArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = bin_row_len(a.lens, b, a.T);
    if (n == 0) {                                                // nothing of this row is read
        if (lane == 0) a.iv_counts[b] = 0;
        return;
    }
    const ulonglong2 *words = reinterpret_cast<const ulonglong2 *>(a.words) + (size_t)b * a.nwt;
    int2 *list = reinterpret_cast<int2 *>(a.list) + (size_t)b * a.cap;
    int *out = a.iv + (size_t)b * a.max_iv * 2;                  // not dereferenced when max_iv is 0; d_iv need not be 8-byte aligned
    const int pon = a.q.pad_on, poff = a.q.pad_off, min_on = a.q.min_on;
    const int D = pon + poff + (a.q.min_off > 1 ? a.q.min_off - 1 : 0), nw = (n + 63) >> 6;
    const ulonglong2 none = make_ulonglong2(0ull, ~0ull);        // past the row: LO
    // the carry, wave-uniform: the state below the pass, one past the last 1 so far (0: none), the last real start (-1: none), intervals kept
    unsigned long long carry = 0;
    int last1 = 0, open_s = -1, niv = 0;
    // [lo, hi) of the interval a real start at s opens, closed at c; true iff it is kept
    auto closes = [&](int s, int c, int &lo, int &hi) {
        lo = s > pon ? s - pon : 0;
        hi = c + poff < n ? c + poff : n;
        return hi - lo >= min_on;
    };
    ulonglong2 next = lane < nw ? words[lane] : none;
    for (int g0 = 0; g0 < nw; g0 += BIN_SPAN_WORDS) {
        const ulonglong2 cur = next;
        if (g0 + BIN_SPAN_WORDS < nw) next = g0 + BIN_SPAN_WORDS + lane < nw ? words[g0 + BIN_SPAN_WORDS + lane] : none;
        const unsigned long long h = cur.x, m = ~(cur.x | cur.y), am = h | m;
        const unsigned long long top0 = (h | (m & ((am + h) ^ am ^ h))) >> 63;   // the word's last state when the state below it is 0
        const unsigned long long gen = __ballot(top0 != 0), prop = __ballot(m == ~0ull), gp = gen | prop;
        const unsigned long long into = (gp + gen + carry) ^ gp ^ gen;           // bit i: the state below word i
        const unsigned long long cin = (into >> lane) & 1ull;
        const unsigned long long x = h | (m & ((am + h + cin) ^ am ^ h));        // the 64 states of this lane's word
        carry = (gen | (prop & into)) >> 63;

        const int f0 = 64 * (g0 + lane);
        const unsigned long long up = __shfl_up(x, 1);
        const unsigned long long pb = lane ? up >> 63 : (unsigned long long)(g0 > 0 && last1 == f0);   // the frame below bit 0
        const unsigned long long rise = x & ~((x << 1) | pb);
        const int top_incl = bin_incl_max(x ? f0 + 64 - __clzll((long long)x) : 0, lane);
        int before = __shfl_up(top_incl, 1);
        before = lane ? (before > last1 ? before : last1) : last1;
        int lr = -1;                                             // the word's last real start
        bin_walk(x, rise, f0, before, D, [&](int s, int) { lr = s; });
        const int lr_incl = bin_incl_max(lr, lane);
        int ps0 = __shfl_up(lr_incl, 1);
        ps0 = lane ? (ps0 > open_s ? ps0 : open_s) : open_s;     // the last real start below this word
        // every real start but the row's first closes the interval its predecessor opened
        int ni = 0, ps = ps0, lo, hi;
        bin_walk(x, rise, f0, before, D, [&](int s, int c) {
            if (c > 0 && closes(ps, c, lo, hi)) ++ni;
            ps = s;
        });
        const int ni_incl = bin_incl_sum(ni, lane);
        int io = niv + ni_incl - ni;
        ps = ps0;
        bin_walk(x, rise, f0, before, D, [&](int s, int c) {
            if (c > 0 && closes(ps, c, lo, hi)) {
                list[io] = make_int2(lo, hi);                    // io < runs of the row <= cap
                if (io < a.max_iv) { out[2 * io] = lo; out[2 * io + 1] = hi; }
                ++io;
            }
            ps = s;
        });
        const int t1 = __shfl(top_incl, 63), l1 = __shfl(lr_incl, 63);
        last1 = t1 > last1 ? t1 : last1;
        open_s = l1 > open_s ? l1 : open_s;
        niv += __shfl(ni_incl, 63);
    }
    if (lane == 0) {
        int lo, hi;
        if (last1 > 0 && closes(open_s, last1, lo, hi)) {        // the row's end closes the last interval
            list[niv] = make_int2(lo, hi);
            if (niv < a.max_iv) { out[2 * niv] = lo; out[2 * niv + 1] = hi; }
            ++niv;
        }
        a.iv_counts[b] = niv;
    }
}

}  // namespace

hipError_t launch_binarize(const BinarizeArgs &a, uint8_t *labels, int ld, hipStream_t s) {
    if (!a.probs || !a.iv_counts || !a.words || reinterpret_cast<uintptr_t>(a.words) % 16 || !a.list || a.B < 1 || a.T < 1 || a.T > BIN_MAX_T || a.ld_p < a.T || a.max_iv < 0 ||
        (a.max_iv > 0 && !a.iv) || a.nwt != bin_words(a.T) || a.cap != (a.T + 1) / 2 || (labels && ld < a.T))
        return hipErrorInvalidValue;
    const int nseg = (a.T + BIN_SEG - 1) / BIN_SEG;
    if ((long long)a.B * nseg > 0x7fffffffll) return hipErrorInvalidValue;
    const bool vec = reinterpret_cast<uintptr_t>(a.probs) % 16 == 0 && (a.B == 1 || a.ld_p % 4 == 0);
    const dim3 grid((unsigned)(a.B * nseg)), block(256);
    if (vec) hipLaunchKernelGGL((binarize_classify_kernel<true>), grid, block, 0, s, a, nseg);
    else hipLaunchKernelGGL((binarize_classify_kernel<false>), grid, block, 0, s, a, nseg);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(binarize_rows_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess || !labels) return e;
    return launch_intervals_to_labels(a.list, a.iv_counts, a.B, a.cap, a.T, ld, a.lens, labels, s);
}

}  // namespace uvad
