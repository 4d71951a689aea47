// endpoint.hip -- the live endpointer (uvad_endpoint_*, include/uvad.h): per feed, the streaming counterpart of median_kernel, runs_kernel
// and the host's merge_intervals_with_buffer, with everything a step depends on held in the device state.
//
// One wave per slot.  A step hands slot b its next n_b probabilities; with m0 frames seen before and m1 = m0 + n_b after, the labels that
// become final are those of frames [max(0, m0 - h), max(0, m1 - h)) (up to m1 on an END step).  The wave lays the thresholded frames out
// as one bit string X in LDS -- the slot's history words (frame m0 - 1 at the top bit of the last one, zeros where the session has no
// frames yet) followed by one __ballot word per 64 new frames, zeros past n_b -- so the zero padding of the offline median at both ends
// of the row is simply the zeros already there.  rank(i) = ones below bit i comes from a per-word prefix of popcounts, and the windowed
// count of a frame is rank(i + h + 1) - rank(i - h): two LDS reads and two popcounts per label, whatever the kernel size.  The labels of
// 64 frames come back as one ballot word and the interval machine walks it with count-trailing-zeros jumps, wave-uniform: it moves only
// at a label change or when a pending run's 2 P frames of silence are complete.
//   launch_endpoint_reset   the header (magic, B, kernel, pad, threshold) by field name and every slot empty, through launch_state_reset
//   endpoint_step_kernel    the step above; writes the slot back and the step's events / counts / active byte / labels
// Plain global loads and stores only; a slot whose count is 0 and whose flags are 0 rewrites its own state unchanged.
#include <climits>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

namespace {

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// cap_words: the 64-bit words of X the launch's LDS holds (the prefix array of cap_words + 1 ints follows them)
__global__ __launch_bounds__(64) void endpoint_step_kernel(EndpointArgs a, int cap_words) {
    extern __shared__ unsigned long long ep_words[];
    const EndpointHeader *hd = reinterpret_cast<const EndpointHeader *>(a.state);
    const int b = blockIdx.x, lane = threadIdx.x;
    if (hd->magic != EP_MAGIC || hd->B != a.B || b >= a.B) return;   // not the state this launch was sized for: touch nothing
    const int K = uni(hd->kernel), P = uni(hd->pad);
    const float thr = hd->threshold;
    const int h = K >> 1, HWn = (2 * h + 63) >> 6, HB = HWn * 64;
    if (K < 1 || HWn > EP_HIST_WORDS || P < 0 || HWn + ((a.ld_in + 63) >> 6) + 1 > cap_words) return;
    int *pc = reinterpret_cast<int *>(ep_words + cap_words);
    EndpointSlot *S = reinterpret_cast<EndpointSlot *>(reinterpret_cast<char *>(a.state) + sizeof(EndpointHeader)) + b;

    const int fl = a.flags ? uni(a.flags[b]) : 0;
    int nb = uni(a.counts[b]);
    nb = nb < 0 ? 0 : nb > a.ld_in ? a.ld_in : nb;
    int m0 = uni(S->m), st = uni(S->st), c = uni(S->c);
    unsigned long long hw = lane < HWn ? S->hist[lane] : 0ull;
    if (fl & UVAD_SLOT_START) { m0 = 0; st = EP_IDLE; c = 0; hw = 0ull; }   // the old session is dropped without events
    if (m0 < 0) m0 = 0;
    if (nb > INT_MAX - m0) nb = INT_MAX - m0;                               // the frame counter saturates: frames past it are not consumed
    const int m1 = m0 + nb;
    const int nwn = (nb + 63) >> 6, W = HWn + nwn + 1;                      // history words, new words, one zero word

    // X: bit HB + k is new frame k; reads stop at n_b
    if (lane < HWn) ep_words[lane] = hw;
    const float *p = a.probs + (size_t)b * a.ld_in;
    for (int j = 0; j < nwn; ++j) {
        const int k = 64 * j + lane;
        bool x = false;
        if (k < nb) x = !(p[k] < thr);                                      // NaN counts as speech, as median_kernel
        const unsigned long long w = __ballot(x);
        if (lane == 0) ep_words[HWn + j] = w;
    }
    if (lane == 0) ep_words[HWn + nwn] = 0ull;
    __syncthreads();
    // pc[w] = ones in words below w
    int carry = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int w = w0 + lane;
        int v = w < W ? __popcll(ep_words[w]) : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o);
            if (lane >= o) v += u;
        }
        if (w < W) pc[w + 1] = carry + v;
        carry += __shfl(v, 63);
    }
    if (lane == 0) pc[0] = 0;
    __syncthreads();

    const bool end = (fl & UVAD_SLOT_END) != 0;
    const int f0 = m0 > h ? m0 - h : 0;
    const int f1 = end ? m1 : (m1 > h ? m1 - h : 0);
    const int nl = f1 - f0;                                                 // 0 .. n_b + h labels become final
    uint8_t *lab = a.labels ? a.labels + (size_t)b * a.ld_lab : nullptr;
    int *ev = (a.events && a.max_events > 0) ? a.events + (size_t)b * a.max_events * 2 : nullptr;
    int nev = 0;
    auto emit = [&](int kind, long long frame) {
        if (lane == 0 && ev && nev < a.max_events) {
            ev[2 * nev] = kind;
            ev[2 * nev + 1] = (int)(frame > INT_MAX ? INT_MAX : frame);
        }
        ++nev;
    };
    auto rank = [&](int i) { return pc[i >> 6] + __popcll(ep_words[i >> 6] & ((1ull << (i & 63)) - 1ull)); };

    for (int j0 = 0; j0 < nl; j0 += 64) {
        const int j = j0 + lane;
        bool y = false;
        if (j < nl) {
            const int i = f0 - m0 + j + HB;                                 // bit of frame f0 + j; i - h >= HB - 2 h >= 0
            const int hi = i + h + 1 < HB + nb ? i + h + 1 : HB + nb;       // bits at and past HB + n_b are zero
            y = rank(hi) - rank(i - h) > h;
            if (lab) lab[j] = y ? 1 : 0;                                    // j < n_b + h <= ld_lab
        }
        const unsigned long long Y = __ballot(y);
        const int nbits = nl - j0 < 64 ? nl - j0 : 64;
        const long long t0 = (long long)f0 + j0;
        // the interval machine over labels t0 .. t0 + nbits - 1 (bits of Y at and past nbits are zero)
        int pos = 0;
        while (pos < nbits) {
            const unsigned long long rem = Y >> pos;
            const int left = nbits - pos;
            if (st == EP_IDLE) {
                if (!rem) break;
                const int k = __builtin_ctzll(rem);
                const long long t = t0 + pos + k;
                emit(1, t > P ? t - P : 0);
                st = EP_SPEECH;
                pos += k + 1;
            } else if (st == EP_SPEECH) {
                const unsigned long long inv = ~rem;
                const int k = inv ? __builtin_ctzll(inv) : 64;
                if (k >= left) break;
                c = (int)(t0 + pos + k);                                    // the zero itself is looked at as pending: P = 0 ends here
                st = EP_PENDING;
                pos += k;
            } else {
                const int k1 = rem ? __builtin_ctzll(rem) : 64;
                const long long texp = (long long)c + 2ll * P;              // a zero at this frame completes the silence
                if (k1 < left && t0 + pos + k1 <= texp) {
                    st = EP_SPEECH;                                         // the run rejoins the pending interval
                    pos += k1 + 1;
                } else if (texp <= t0 + nbits - 1) {
                    emit(2, (long long)c + P);
                    st = EP_IDLE;
                    const long long np = texp - t0 + 1;
                    pos = np > pos ? (int)np : pos;
                } else {
                    break;
                }
            }
        }
    }
    if (end) {
        if (st == EP_SPEECH) emit(2, m1);
        else if (st == EP_PENDING) emit(2, (long long)c + P < m1 ? (long long)c + P : m1);
        st = EP_IDLE;
        c = 0;
    }
    // the slot's next state: the newest HB bits of X, or the empty session
    if (lane < EP_HIST_WORDS) {
        unsigned long long v = 0ull;
        if (!end && lane < HWn) {
            const int o = nb + 64 * lane, q = o >> 6, r = o & 63;           // q + 1 <= W - 1
            v = r ? (ep_words[q] >> r) | (ep_words[q + 1] << (64 - r)) : ep_words[q];
        }
        S->hist[lane] = v;
    }
    if (lane == 0) {
        S->m = end ? 0 : m1;
        S->st = st;
        S->c = c;
        a.ev_counts[b] = nev;
        if (a.active) a.active[b] = st != EP_IDLE ? 1 : 0;
        if (a.lab_counts) a.lab_counts[b] = nl;
    }
}

int endpoint_cap_words(int kernel, int ld_in) { return ((kernel / 2 * 2 + 63) >> 6) + ((ld_in + 63) >> 6) + 1; }

}  // namespace

size_t endpoint_state_bytes(int B) { return sizeof(EndpointHeader) + (size_t)B * sizeof(EndpointSlot); }

hipError_t launch_endpoint_reset(void *state, int B, int kernel, int pad, float threshold, hipStream_t s) {
    if (!state || B <= 0) return hipErrorInvalidValue;
    EndpointHeader h{};
    h.magic = EP_MAGIC; h.B = B; h.kernel = kernel; h.pad = pad; h.threshold = threshold;
    return launch_state_reset(state, header_words(h), (long long)(endpoint_state_bytes(B) / sizeof(unsigned)), s);
}

hipError_t launch_endpoint_step(const EndpointArgs &a, int kernel, hipStream_t s) {
    if (!a.probs || !a.counts || !a.state || !a.ev_counts || a.B <= 0 || a.ld_in < 1 || a.ld_in > EP_MAX_LD_IN || kernel < 1 || kernel > 255)
        return hipErrorInvalidValue;
    const int cap = endpoint_cap_words(kernel, a.ld_in);
    const size_t lds = (size_t)cap * sizeof(unsigned long long) + (size_t)(cap + 1) * sizeof(int);
    hipLaunchKernelGGL(endpoint_step_kernel, dim3((unsigned)a.B), dim3(64), lds, s, a, cap);
    return hipGetLastError();
}

}  // namespace uvad
