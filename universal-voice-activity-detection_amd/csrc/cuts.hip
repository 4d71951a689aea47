// cuts.hip -- speech cuts on the device (uvad_cuts_*, include/uvad.h): the offline counterpart of endpoint.hip.  Label rows -> the runs,
// widened by P frames and merged (merge_intervals_with_buffer in frames, postprocess.merged_runs), split into pieces of at most W frames
// (split_into_windows on integers, src/scripts/predict.py:638-647), each piece with its sample range; then the audio (or the feature
// frames) of every cut gathered into a zero-padded batch with lengths.  All integer, no atomics: the same calls give the same bytes.
//
// The padded merge is a closing followed by a dilation: runs [s, c) and [s', c') merge iff s' - c <= 2 P (the clipping at 0 and n never
// changes that), so a run start is REAL -- it opens a merged interval -- iff it is the row's first or its zero gap is longer than 2 P,
// and the interval that a real start at s opens is [max(s - P, 0), min(c + P, n)) with c one past the last 1 before the next real start
// (or before the row's end).  A real start therefore closes its predecessor's interval, and needs for that only two prefix maxima: the
// last 1 before it and the last real start before it.
//   cuts_rows_kernel    one workgroup of five waves per row.  The row goes by in passes of CUTS_SPAN_WORDS __ballot words (64 frames
//                       each, zeros past len_b): four waves make the words of the next pass while wave 0 works on this one, one word
//                       per lane: run starts by bit operations, the last 1 below each by count-leading-zeros, the two prefix maxima and
//                       the output positions by wave scans, the real starts of a word by count-trailing-zeros jumps.  What a pass leaves
//                       to the next is four integers in wave 0's registers.  Out: the row's merged intervals that keep at least one
//                       piece {lo, hi, index of the first piece within the row}, their number and the row's number of cuts, in the
//                       workspace.
//   cuts_scan_kernel    one workgroup: the exclusive prefix of the rows' cut counts (256 rows per round, carried) -> d_row_first, d_total
//   cuts_write_kernel   one thread per cut below min(total, max_cuts): its row and its interval by two binary searches, the piece and
//                       its sample range in closed form, stored at its global index
//   cuts_gather_kernel  one workgroup per (cut, tile of CUTS_TILE_BYTES of the output row) pair at a time, pairs past the device's total
//                       never started: 16-byte stores to the output row (aligned on the destination side; a cut starts at any sample),
//                       plain loads of the source's own granule (2 or 4 bytes) from the cut's range alone, zeros past its end in the
//                       same pass.  A granule-wide form serves output rows whose byte stride is no multiple of 16.
#include <cstddef>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

static_assert(sizeof(uvad_cut) == 32 && sizeof(CutRecord) == 32 && sizeof(uvad_cuts_cfg) == 24 && sizeof(CutsCfgInt) == 24 && sizeof(CutsInterval) == 16,
              "the records of include/uvad.h and the workspace");
static_assert(offsetof(uvad_cut, n_frames) == offsetof(CutRecord, n_frames) && offsetof(uvad_cut, n_samples) == offsetof(CutRecord, n_samples), "uvad_cut");
static_assert(CUTS_MAX_T == (1 << 30) && CUTS_SPAN_WORDS == 64 && CUTS_ROWS_THREADS == 320, "frame arithmetic in int32; one word per lane of wave 0, four loading waves");

namespace {

__device__ __forceinline__ int wave_incl_max(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v = u > v ? u : v;
    }
    return v;
}

__device__ __forceinline__ int wave_incl_sum(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// pieces an interval of L >= 1 frames keeps: q = (L - 1) / W full ones and the last of r = L - q W frames iff r > m (W = 0: q = 0, r = L)
__host__ __device__ __forceinline__ int cuts_pieces(int L, int W, int m) {
    const int q = W ? (L - 1) / W : 0;
    return q + (L - q * W > m ? 1 : 0);
}

// the real starts among the run starts `rise` of the word x (frames f0 .. f0 + 63), in ascending order: f(s, c) with c one past the last 1
// before s (0: the row's first run); `before` is that for the words below this one
template <class F> __device__ __forceinline__ void cuts_walk(unsigned long long x, unsigned long long rise, int f0, int before, int twoP, F &&f) {
    while (rise) {
        const int i = __builtin_ctzll(rise);
        rise &= rise - 1ull;
        const unsigned long long below = x & ((1ull << i) - 1ull);
        const int c = below ? f0 + 64 - __clzll((long long)below) : before;
        if (c == 0 || f0 + i - c > twoP) f(f0 + i, c);
    }
}

__global__ __launch_bounds__(CUTS_ROWS_THREADS) void cuts_rows_kernel(CutsTableArgs a) {
    __shared__ unsigned long long words[2][CUTS_SPAN_WORDS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = a.T;
    if (a.lens) { n = a.lens[b]; n = n < 0 ? 0 : n > a.T ? a.T : n; }
    if (n == 0) {                                                // nothing of this row is read
        if (tid == 0) a.counts[2 * b] = a.counts[2 * b + 1] = 0;
        return;
    }
    const uint8_t *row = a.labels + (size_t)b * a.ld;
    CutsInterval *iv = a.iv + (size_t)b * a.cap;
    const int P = a.q.pad, W = a.q.max_len, m = a.q.min_len, nw = (n + 63) >> 6;
    // wave 0's carry, wave-uniform: one past the last 1 so far (0: none), the last real start (-1: none), intervals and cuts stored so far
    int last1 = 0, open_s = -1, niv = 0, ncut = 0;
    // Waves 1 .. 4 make the words of pass p (16 each) in buffer p & 1 before barrier p; wave 0 reads them after it, while the others are
    // already loading pass p + 1 into the other buffer.  Buffer p & 1 is written again only after barrier p + 1, which wave 0 reaches when
    // it is done with pass p: one barrier per pass.
    for (int g0 = 0, buf = 0; g0 < nw; g0 += CUTS_SPAN_WORDS, buf ^= 1) {
        if (wave > 0) {
            constexpr int PER = CUTS_SPAN_WORDS / 4;
            const int j0 = PER * (wave - 1);
            uint8_t v[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) {                      // all loads first, then the ballots
                const int f = 64 * (g0 + j0 + k) + lane;         // < 2^30 + 64 * CUTS_SPAN_WORDS
                v[k] = f < n ? row[f] : (uint8_t)0;              // columns at or past len_b are never read
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const unsigned long long w = __ballot(v[k] != 0);
                if (lane == 0) words[buf][j0 + k] = w;
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int f0 = 64 * (g0 + lane);
            const unsigned long long x = words[buf][lane], up = __shfl_up(x, 1);
            const unsigned long long pb = lane ? up >> 63 : (unsigned long long)(g0 > 0 && last1 == f0);   // the frame below bit 0
            const unsigned long long rise = x & ~((x << 1) | pb);
            const int top_incl = wave_incl_max(x ? f0 + 64 - __clzll((long long)x) : 0, lane);
            int before = __shfl_up(top_incl, 1);
            before = lane ? (before > last1 ? before : last1) : last1;
            int lr = -1;                                         // the word's last real start
            cuts_walk(x, rise, f0, before, 2 * P, [&](int s, int) { lr = s; });
            const int lr_incl = wave_incl_max(lr, lane);
            int ps0 = __shfl_up(lr_incl, 1);
            ps0 = lane ? (ps0 > open_s ? ps0 : open_s) : open_s; // the last real start below this word
            // every real start but the row's first closes the interval its predecessor opened
            int ni = 0, nc = 0, ps = ps0;
            cuts_walk(x, rise, f0, before, 2 * P, [&](int s, int c) {
                if (c > 0) {
                    const int lo = ps > P ? ps - P : 0, hi = c + P < n ? c + P : n, k = cuts_pieces(hi - lo, W, m);
                    if (k) { ++ni; nc += k; }
                }
                ps = s;
            });
            const int ni_incl = wave_incl_sum(ni, lane), nc_incl = wave_incl_sum(nc, lane);
            int io = niv + ni_incl - ni, co = ncut + nc_incl - nc;
            ps = ps0;
            cuts_walk(x, rise, f0, before, 2 * P, [&](int s, int c) {
                if (c > 0) {
                    const int lo = ps > P ? ps - P : 0, hi = c + P < n ? c + P : n, k = cuts_pieces(hi - lo, W, m);
                    if (k) { iv[io] = CutsInterval{lo, hi, co, 0}; ++io; co += k; }   // io < runs of the row <= cap
                }
                ps = s;
            });
            const int t1 = __shfl(top_incl, 63), l1 = __shfl(lr_incl, 63);
            last1 = t1 > last1 ? t1 : last1;
            open_s = l1 > open_s ? l1 : open_s;
            niv += __shfl(ni_incl, 63);
            ncut += __shfl(nc_incl, 63);
        }
    }
    if (tid == 0) {
        if (last1 > 0) {                                         // the row's end closes the last interval
            const int lo = open_s > P ? open_s - P : 0, hi = last1 + P < n ? last1 + P : n, k = cuts_pieces(hi - lo, W, m);
            if (k) { iv[niv] = CutsInterval{lo, hi, ncut, 0}; ++niv; ncut += k; }
        }
        a.counts[2 * b] = ncut;
        a.counts[2 * b + 1] = niv;
    }
}

__global__ __launch_bounds__(256) void cuts_scan_kernel(const int *counts, int B, int *row_first, int *total) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + tid, v = b < B ? counts[2 * b] : 0;
        const int incl = wave_incl_sum(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int off = 0;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (b < B) row_first[b] = carry + off + incl - v;
        carry += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        __syncthreads();
    }
    if (tid == 0) { row_first[B] = carry; *total = carry; }
}

__global__ __launch_bounds__(256) void cuts_write_kernel(CutsTableArgs a) {
    const int total = a.row_first[a.B], lim = total < a.max_cuts ? total : a.max_cuts;
    const int W = a.q.max_len;
    for (long long i0 = (long long)blockIdx.x * 256 + threadIdx.x; i0 < lim; i0 += (long long)gridDim.x * 256) {
        const int i = (int)i0;
        int b = 0, hi = a.B;                                     // row_first[b] <= i < row_first[hi]; rows without cuts repeat their successor's entry
        while (hi - b > 1) {
            const int mid = (b + hi) >> 1;
            if (a.row_first[mid] <= i) b = mid; else hi = mid;
        }
        const int k = i - a.row_first[b];
        const CutsInterval *iv = a.iv + (size_t)b * a.cap;
        int j = 0;
        hi = a.counts[2 * b + 1];                                // iv[j].base <= k < iv[hi].base (bases ascend strictly)
        while (hi - j > 1) {
            const int mid = (j + hi) >> 1;
            if (iv[mid].base <= k) j = mid; else hi = mid;
        }
        const CutsInterval v = iv[j];
        const int p = k - v.base, L = v.hi - v.lo, q = W ? (L - 1) / W : 0;
        long long Sb = a.S;
        if (a.nsamp) { Sb = a.nsamp[b]; Sb = Sb < 0 ? 0 : Sb > a.S ? a.S : Sb; }
        CutRecord c;
        c.row = b;
        c.index = k;
        c.first_frame = v.lo + p * W;                            // p W < L
        c.n_frames = p < q ? W : L - q * W;
        long long s0 = (long long)c.first_frame * a.q.hop - a.q.lead, s1 = ((long long)c.first_frame + c.n_frames) * a.q.hop + a.q.tail;
        s0 = s0 < 0 ? 0 : s0;
        s1 = s1 > Sb ? Sb : s1;
        c.first_sample = s0;
        c.n_samples = s1 > s0 ? s1 - s0 : 0;
        a.table[i] = c;
    }
}

// G: the source's granule (uint16_t: int16 samples; uint32_t: f32 samples and feature records); VEC: 16-byte stores
template <class G, bool VEC> __global__ __launch_bounds__(256) void cuts_gather_kernel(CutsGatherArgs a) {
    constexpr long long TILE = CUTS_TILE_BYTES / sizeof(G);      // granules per tile
    constexpr int V = 16 / sizeof(G);
    const int total = *a.total, lim = total < a.max_cuts ? total : a.max_cuts, tid = threadIdx.x;
    const long long pairs = (long long)lim * a.tiles, gper = a.unit_bytes / (int)sizeof(G), row_g = a.ld_out * gper;
    for (long long pr = blockIdx.x; pr < pairs; pr += gridDim.x) {
        const int cut = (int)(pr / a.tiles), tile = (int)(pr % a.tiles);
        const CutRecord q = a.table[cut];
        const long long first = a.frames ? (long long)q.first_frame : q.first_sample;
        long long c = a.frames ? (long long)q.n_frames : q.n_samples;
        c = c > a.ld_out ? a.ld_out : c;
        if (q.row < 0 || first < 0) c = 0;                       // not a table uvad_cuts_table wrote: nothing is read outside the source row
        else if (c > a.row_stride - first) c = a.row_stride - first;
        c = c < 0 ? 0 : c;
        if (tile == 0 && tid == 0) a.out_len[cut] = (int)c;
        const long long copy_g = c * gper;
        const G *src = reinterpret_cast<const G *>(a.src) + ((long long)q.row * a.row_stride + first) * gper;
        G *dst = reinterpret_cast<G *>(a.out) + (long long)cut * row_g;
        const long long g0 = tile * TILE, g1 = g0 + TILE < row_g ? g0 + TILE : row_g;
        if (VEC) {                                               // row_g is a multiple of V and dst is 16-byte aligned
            for (long long g = g0 + (long long)tid * V; g < g1; g += 256 * V) {
                union { G e[V]; uint4 v; } u;
                if (g + V <= copy_g) {
#pragma unroll
                    for (int k = 0; k < V; ++k) u.e[k] = src[g + k];
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) u.e[k] = g + k < copy_g ? src[g + k] : (G)0;
                }
                *reinterpret_cast<uint4 *>(dst + g) = u.v;
            }
        } else {
            for (long long g = g0 + tid; g < g1; g += 256) dst[g] = g < copy_g ? src[g] : (G)0;
        }
    }
}

}  // namespace

int cuts_max_per_row(const CutsCfgInt &q, int T) { return (T + 1) / 2 + (q.max_len ? T / q.max_len : 0); }

hipError_t launch_cuts_table(const CutsTableArgs &a, hipStream_t s) {
    if (!a.labels || !a.row_first || !a.total || !a.counts || !a.iv || a.B < 1 || a.T < 1 || a.T > CUTS_MAX_T || a.ld < a.T || a.S < 0 ||
        a.max_cuts < 0 || (a.max_cuts > 0 && !a.table) || a.cap != (a.T + 1) / 2 || (long long)a.B * cuts_max_per_row(a.q, a.T) > 0x7fffffffll)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(cuts_rows_kernel, dim3((unsigned)a.B), dim3(CUTS_ROWS_THREADS), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cuts_scan_kernel, dim3(1), dim3(256), 0, s, a.counts, a.B, a.row_first, a.total);
    e = hipGetLastError();
    if (e != hipSuccess || a.max_cuts == 0) return e;
    long long most = (long long)a.B * cuts_max_per_row(a.q, a.T);
    most = most < a.max_cuts ? most : a.max_cuts;
    long long blocks = (most + 255) / 256;
    blocks = blocks > CUTS_MAX_BLOCKS ? CUTS_MAX_BLOCKS : blocks;
    hipLaunchKernelGGL(cuts_write_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_cuts_gather(const CutsGatherArgs &a, hipStream_t s) {
    const int g = a.frames || a.unit_bytes == 4 ? 4 : 2;
    if (!a.src || !a.table || !a.total || !a.out || !a.out_len || a.max_cuts < 0 || a.ld_out < 1 || a.ld_out > 0x7fffffffll || a.row_stride < 0 ||
        a.unit_bytes < 2 || a.unit_bytes > 4096 || a.unit_bytes % g || (!a.frames && a.unit_bytes != 2 && a.unit_bytes != 4) ||
        a.tiles != cuts_gather_tiles(a.ld_out, a.unit_bytes))
        return hipErrorInvalidValue;
    if (a.max_cuts == 0) return hipSuccess;
    long long blocks = (long long)a.max_cuts * a.tiles;
    blocks = blocks > CUTS_MAX_BLOCKS ? CUTS_MAX_BLOCKS : blocks;
    const bool vec = (a.ld_out * a.unit_bytes) % 16 == 0 && reinterpret_cast<uintptr_t>(a.out) % 16 == 0;
    const dim3 grid((unsigned)blocks), block(256);
    if (g == 2) {
        if (vec) hipLaunchKernelGGL((cuts_gather_kernel<uint16_t, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cuts_gather_kernel<uint16_t, false>), grid, block, 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((cuts_gather_kernel<uint32_t, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cuts_gather_kernel<uint32_t, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace uvad
