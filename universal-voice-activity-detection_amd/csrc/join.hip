// join.hip -- the cut-supervision join on the device (uvad_cuts_join, include/uvad.h): the step the reference's get_new_cuts exists for
// (src/scripts/predict.py:515-572, the counters of :597-611).  A cut table as uvad_cuts_table wrote it and, per row, a list of items {s, e}
// in frames (supervisions, or the words of an alignment) -> for every cut the items of its row that it matches, in ascending item order,
// for every item the run of cuts that match it, and eight counters per row.  All integer, no atomics: the same calls give the same bytes.
//
// A cut covers [f, f + k); an item is [s, e), and one with e <= s matches nothing.  OVERLAP: s < f + k and e > f.  INSIDE: s >= f and
// e <= f + k.  A row's cuts ascend and are disjoint, so in either mode the cuts an item matches are a run: "the cut reaches far enough"
// holds on a suffix of the row's cuts and "the cut starts early enough" on a prefix.
//   join_items_kernel  one workgroup per row, threads striding over the row's items: the two bounds by binary searches over the row's
//                      cuts -> d_item_cuts {first, n}; the exceeding pairs of an item are those of its first and last cut, looked at,
//                      plus every cut strictly between (such a cut starts past s).  Wave and workgroup sums leave words 0, 3, 4, 5.
//   join_count_kernel  one wave per cut: the row's items go by 64 at a time, one per lane; __ballot and a population count -> the
//                      cut's number of pairs, in the workspace.  Nothing of the items kernel is used: the two sides agree or a test fails.
//   join_scan_kernel   one workgroup: the exclusive prefixes of the cuts' pairs (-> d_pair_first) and of the cuts without a pair
//                      (-> workspace), 256 cuts per round, carried; then one thread per row finishes words 1, 2, 6, 7 by subtraction
//                      and the workgroup sums row B.
//   join_write_kernel  one wave per cut: the same walk, each matching lane's rank below it in the ballot -> d_pairs from the cut's
//                      d_pair_first on, below max_pairs.
// The cost is cuts x items of a row, 64 items a step; items are unsorted by contract, so no cut can skip any of them.
#include <cstddef>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

static_assert(JOIN_AUDIT_WORDS == UVAD_JOIN_AUDIT_WORDS && UVAD_JOIN_OVERLAP == 0 && UVAD_JOIN_INSIDE == 1, "include/uvad.h");

namespace {

typedef unsigned long long u64;

// the cuts that take part: global indices below m; row b's are [c0, c1)
__device__ __forceinline__ int join_m(const JoinArgs &a) {
    const int t = *a.total;
    return t < 0 ? 0 : t < a.max_cuts ? t : a.max_cuts;
}
__device__ __forceinline__ void join_row_cuts(const JoinArgs &a, int b, int m, int &c0, int &c1) {
    c0 = a.row_first[b];
    c1 = a.row_first[b + 1];
    c0 = c0 < 0 ? 0 : c0 > m ? m : c0;
    c1 = c1 < c0 ? c0 : c1 > m ? m : c1;
}
__device__ __forceinline__ int join_row_items(const JoinArgs &a, int b) {
    const int n = a.iv_counts[b];
    return n < 0 ? 0 : n > a.max_iv ? a.max_iv : n;
}

__device__ __forceinline__ bool join_match(bool inside, long long f, long long c, long long s, long long e) {   // the cut [f, c), the item [s, e)
    return e > s && (inside ? (s >= f && e <= c) : (s < c && e > f));
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                                    // lane 0 holds the sum
}

__global__ __launch_bounds__(256) void join_items_kernel(JoinArgs a) {
    __shared__ long long part[4][2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = join_m(a), nb = join_row_items(a, b);
    int c0, c1;
    join_row_cuts(a, b, m, c0, c1);
    const bool inside = a.inside != 0;
    long long matched = 0, exceed = 0;
    for (int j = tid; j < nb; j += 256) {
        const size_t at = ((size_t)b * a.max_iv + j) * 2;
        int first = -1, n = 0;
        if (c1 > c0) {                                           // the item slots of a row without cuts are never read
            const long long s = a.iv[at], e = a.iv[at + 1];
            if (e > s) {
                // lo: the first cut that reaches far enough (OVERLAP: f + k > s; INSIDE: f + k >= e)
                int lo = c0, hi = c1;
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    const CutRecord q = a.table[mid];
                    const long long c = (long long)q.first_frame + q.n_frames;
                    if (inside ? c >= e : c > s) hi = mid; else lo = mid + 1;
                }
                // up: the first cut that starts too late (OVERLAP: f >= e; INSIDE: f > s)
                int up = lo;
                hi = c1;
                while (up < hi) {
                    const int mid = up + ((hi - up) >> 1);
                    const long long f = a.table[mid].first_frame;
                    if (inside ? f > s : f >= e) hi = mid; else up = mid + 1;
                }
                if (up > lo) {
                    first = lo;
                    n = up - lo;
                    const CutRecord q0 = a.table[lo], q1 = a.table[up - 1];
                    const bool x0 = q0.first_frame > s || (long long)q0.first_frame + q0.n_frames < e;
                    const bool x1 = q1.first_frame > s || (long long)q1.first_frame + q1.n_frames < e;
                    exceed += (x0 ? 1 : 0) + (n > 1 ? (x1 ? 1 : 0) + (n - 2) : 0);
                    ++matched;
                }
            }
        }
        if (a.item_cuts) { a.item_cuts[at] = first; a.item_cuts[at + 1] = n; }
    }
    matched = wave_sum(matched);
    exceed = wave_sum(exceed);
    if (lane == 0) { part[wave][0] = matched; part[wave][1] = exceed; }
    __syncthreads();
    if (tid == 0) {
        const long long mt = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]), ex = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
        u64 *w = a.audit + (size_t)b * JOIN_AUDIT_WORDS;
        w[0] = (u64)nb;
        w[3] = (u64)mt;
        w[4] = (u64)(nb - mt);
        w[5] = (u64)ex;
    }
}

// the walk of one wave over its cut's row: f(j, match, ballot) per step of 64 items, item j = j0 + lane (match is false past the row's count)
template <class F> __device__ __forceinline__ void join_walk(const JoinArgs &a, int i, int lane, F &&f) {
    const CutRecord q = a.table[i];
    if (q.row < 0 || q.row >= a.B) return;                      // not a table uvad_cuts_table wrote
    const int nb = join_row_items(a, q.row);
    const long long lo = q.first_frame, c = lo + q.n_frames;
    const int *iv = a.iv + (size_t)q.row * a.max_iv * 2;
    const bool inside = a.inside != 0;
    for (int j0 = 0; j0 < nb; j0 += 64) {
        const int j = j0 + lane;                                 // j0 is a multiple of 64 below 2^31 - 1, so j0 + 63 fits
        bool hit = false;
        if (j < nb) {                                            // slots at or past the row's count are never read
            const long long s = iv[(size_t)j * 2], e = iv[(size_t)j * 2 + 1];
            hit = join_match(inside, lo, c, s, e);
        }
        f(j, hit, (u64)__ballot(hit));
    }
}

__global__ __launch_bounds__(256) void join_count_kernel(JoinArgs a) {
    const int lane = threadIdx.x & 63, m = join_m(a);
    for (long long i0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i0 < m; i0 += (long long)gridDim.x * 4) {
        int n = 0;
        join_walk(a, (int)i0, lane, [&](int, bool, u64 mask) { n += __popcll(mask); });
        if (lane == 0) a.counts[i0] = n;
    }
}

__global__ __launch_bounds__(256) void join_scan_kernel(JoinArgs a) {
    __shared__ int wsum[4][2];
    __shared__ long long rsum[4][JOIN_AUDIT_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = join_m(a);
    int carry = 0, carry0 = 0;
    for (int i0 = 0; i0 < m; i0 += 256) {
        const int i = i0 + tid, v = i < m ? a.counts[i] : 0, z = i < m && v == 0 ? 1 : 0;
        int incl = v, incl0 = z;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o), u0 = __shfl_up(incl0, o);
            if (lane >= o) { incl += u; incl0 += u0; }
        }
        if (lane == 63) { wsum[wave][0] = incl; wsum[wave][1] = incl0; }
        __syncthreads();
        int off = 0, off0 = 0;
        for (int w = 0; w < wave; ++w) { off += wsum[w][0]; off0 += wsum[w][1]; }
        if (i < m) { a.pair_first[i] = carry + off + incl - v; a.empty_first[i] = carry0 + off0 + incl0 - z; }
        carry += (wsum[0][0] + wsum[1][0]) + (wsum[2][0] + wsum[3][0]);
        carry0 += (wsum[0][1] + wsum[1][1]) + (wsum[2][1] + wsum[3][1]);
        __syncthreads();
    }
    if (tid == 0) { a.pair_first[m] = carry; a.empty_first[m] = carry0; }
    __syncthreads();                                             // the two prefixes are read below by other threads of this workgroup
    long long sum[JOIN_AUDIT_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = tid; b < a.B; b += 256) {
        int c0, c1;
        join_row_cuts(a, b, m, c0, c1);
        u64 *w = a.audit + (size_t)b * JOIN_AUDIT_WORDS;            // words 0, 3, 4, 5 are join_items_kernel's
        const long long pairs = (long long)a.pair_first[c1] - a.pair_first[c0];
        w[1] = (u64)(c1 - c0);
        w[2] = (u64)pairs;
        w[6] = (u64)(pairs - (long long)w[3]);
        w[7] = (u64)(a.empty_first[c1] - a.empty_first[c0]);
#pragma unroll
        for (int k = 0; k < JOIN_AUDIT_WORDS; ++k) sum[k] += (long long)w[k];
    }
#pragma unroll
    for (int k = 0; k < JOIN_AUDIT_WORDS; ++k) {
        const long long v = wave_sum(sum[k]);
        if (lane == 0) rsum[wave][k] = v;
    }
    __syncthreads();
    if (tid < JOIN_AUDIT_WORDS)
        a.audit[(size_t)a.B * JOIN_AUDIT_WORDS + tid] = (u64)((rsum[0][tid] + rsum[1][tid]) + (rsum[2][tid] + rsum[3][tid]));
}

__global__ __launch_bounds__(256) void join_write_kernel(JoinArgs a) {
    const int lane = threadIdx.x & 63, m = join_m(a);
    const u64 below = (1ull << lane) - 1ull;
    for (long long i0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i0 < m; i0 += (long long)gridDim.x * 4) {
        long long at = a.pair_first[i0];                         // wave-uniform; pairs at or past max_pairs are counted, not stored
        join_walk(a, (int)i0, lane, [&](int j, bool hit, u64 mask) {
            const long long mine = at + __popcll(mask & below);
            if (hit && mine < a.max_pairs) a.pairs[mine] = j;
            at += __popcll(mask);
        });
    }
}

}  // namespace

hipError_t launch_cuts_join(const JoinArgs &a, hipStream_t s) {
    if (!a.row_first || !a.total || !a.iv_counts || !a.pair_first || !a.audit || !a.counts || !a.empty_first || a.B < 1 || a.max_iv < 0 ||
        a.max_cuts < 0 || a.max_pairs < 0 || (a.max_cuts > 0 && !a.table) || (a.max_iv > 0 && !a.iv) || (a.max_pairs > 0 && !a.pairs) ||
        (long long)a.max_cuts * a.max_iv > 0x7fffffffll)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(join_items_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    long long blocks = ((long long)a.max_cuts + 3) / 4;          // one wave per cut, strided past the cap
    blocks = blocks > CUTS_MAX_BLOCKS ? CUTS_MAX_BLOCKS : blocks;
    if (blocks > 0) {
        hipLaunchKernelGGL(join_count_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(join_scan_kernel, dim3(1), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess || blocks == 0 || a.max_pairs == 0) return e;
    hipLaunchKernelGGL(join_write_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
