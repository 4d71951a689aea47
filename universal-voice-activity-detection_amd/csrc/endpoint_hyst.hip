// endpoint_hyst.hip -- the live hysteresis endpointer (uvad_endpoint_hyst_*, include/uvad.h): per feed, uvad_binarize's decisions (two
// thresholds, a shortest speech interval, a shortest pause, asymmetric padding) as START / END events and final labels, with everything
// a step depends on held in the device state.
//
// One wave per slot.  The hysteresis state s[t] is causal -- known the moment frame t arrives -- so a slot keeps no frames: its state is
// seven integers (EndpointHystSlot).  Per 64 new frames the wave builds two __ballot words, HI and LO (frames at or past n_b go neither
// way: they are MID, so the carry out of the word is the state of the last real frame, and they are never walked), and gets the 64
// states from the one addition binarize.hip documents: a = HI | MID, b = HI, carry-in = the slot's state bit.  The interval machine of
// the header's six rules then walks that word wave-uniformly.  A frame changes nothing -- it is "boring" -- when
//   IDLE                     s = 0
//   SPEECH, confirmed        s = 1
//   SPEECH, unconfirmed      s = 1 and the interval still has fewer than min_on frames:  t + 1 - lo < min_on
//   PENDING, confirmed       s = 0 and the D frames of silence are not complete:  t < c + D
//   PENDING, unconfirmed     the same, and min(c + pad_off, t + 1) - lo < min_on
// so the walk jumps with count-trailing-zeros to the next state change, caps the jump at the one frame that completes the silence or
// confirms the candidate, and applies the rules, as written, to that frame alone.  Applying them to a boring frame would be harmless;
// skipping a frame that is not boring is the only way to go wrong, and the five lines above are all there is to check.
// Labels: what a step finalises is a few constant segments -- zeros while idle (up to m - pad_on), ones while a confirmed interval runs,
// [lo, hi) at once when a candidate is confirmed or dropped -- and the frontier only moves forward, so before every frame the walk stops
// at, and once after the last, the lanes fill [F, new F) with one value.
//   launch_endpoint_hyst_reset   the header (magic, B, the uvad_binarize_cfg) by field name and every slot empty, through launch_state_reset
//   endpoint_hyst_step_kernel    the step above; writes the slot back and the step's events / counts / active byte / labels
// No LDS, no atomics, plain global loads and stores; a slot whose count is 0 and whose flags are 0 rewrites its own state unchanged.
#include <climits>
#include "uvad_internal.h"
#include "../../include/uvad.h"

namespace uvad {

static_assert(sizeof(EndpointHystHeader) == 256 && sizeof(EndpointHystSlot) == 32 && sizeof(BinCfgInt) == sizeof(uvad_binarize_cfg), "uvad_endpoint_hyst state");

namespace {

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(64) void endpoint_hyst_step_kernel(EndpointArgs a) {
    const EndpointHystHeader *hd = reinterpret_cast<const EndpointHystHeader *>(a.state);
    const int b = blockIdx.x, lane = threadIdx.x;
    if (hd->magic != EPH_MAGIC || hd->B != a.B || b >= a.B) return;       // not the state this launch was sized for: touch nothing
    const float on = hd->q.onset, off = hd->q.offset;
    const int min_on = uni(hd->q.min_on), min_off = uni(hd->q.min_off), pon = uni(hd->q.pad_on), poff = uni(hd->q.pad_off);
    if (min_on < 0 || min_on > BIN_MAX_FRAMES || min_off < 0 || min_off > BIN_MAX_FRAMES || pon < 0 || pon > BIN_MAX_FRAMES || poff < 0 ||
        poff > BIN_MAX_FRAMES)
        return;
    const long long D = (long long)pon + poff + (min_off > 1 ? min_off - 1 : 0);
    EndpointHystSlot *S = reinterpret_cast<EndpointHystSlot *>(reinterpret_cast<char *>(a.state) + sizeof(EndpointHystHeader)) + b;

    const int fl = a.flags ? uni(a.flags[b]) : 0;
    int nb = uni(a.counts[b]);
    nb = nb < 0 ? 0 : nb > a.ld_in ? a.ld_in : nb;
    int m0 = uni(S->m), mode = uni(S->mode), conf = uni(S->conf), s = uni(S->s) & 1;
    long long F = uni(S->F), lo = uni(S->lo), c = uni(S->c);                // positions such as c + pad_off are formed in 64 bits
    if (fl & UVAD_SLOT_START) { m0 = 0; mode = EP_IDLE; conf = 0; s = 0; F = 0; lo = 0; c = 0; }   // the old session is dropped without events
    if (m0 < 0) m0 = 0;
    if (nb > INT_MAX - m0) nb = INT_MAX - m0;                               // the frame counter saturates: frames past it are not consumed
    const int m1 = m0 + nb;
    const long long F0 = F;

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
    // labels [F, upto) become final with one value; output column = frame - F0, never past ld_lab
    auto fill = [&](int value, long long upto) {
        if (upto <= F) return;
        if (lab) {
            const long long o1 = upto - F0 < a.ld_lab ? upto - F0 : a.ld_lab;
            for (long long o = F - F0 + lane; o < o1; o += 64) lab[o] = (uint8_t)value;
        }
        F = upto;
    };
    // rule 5 over the boring frames up to m = mm: the frontier is monotone in m while the mode stands
    auto advance = [&](long long mm) {
        if (mode == EP_IDLE) fill(0, mm - pon);
        else if (conf) fill(1, mode == EP_SPEECH ? mm : (c + poff < mm ? c + poff : mm));
    };
    // rules 2 .. 4 for frame t with state bit sb
    auto frame = [&](long long t, bool sb) {
        if (mode == EP_IDLE && sb) {
            lo = t > pon ? t - pon : 0;
            mode = EP_SPEECH;
            conf = 0;
        } else if (mode == EP_SPEECH && !sb) {
            c = t;
            mode = EP_PENDING;
        } else if (mode == EP_PENDING && sb) {
            mode = EP_SPEECH;                                               // the run rejoins with no event
        }
        if (mode == EP_PENDING && !sb && t >= c + D) {
            const long long hi = c + poff;
            if (conf) emit(2, hi);
            fill(conf, hi);                                                 // [lo, hi): ones if kept, zeros if dropped
            mode = EP_IDLE;
            conf = 0;
        }
        if (mode != EP_IDLE && !conf) {
            const long long m = t + 1, e = c + poff;
            const long long bound = mode == EP_SPEECH ? m : (e < m ? e : m);
            if (bound - lo >= min_on) {
                emit(1, lo);
                conf = 1;
            }
        }
    };

    const float *p = a.probs + (size_t)b * a.ld_in;
    const int nwn = (nb + 63) >> 6;
    float next = lane < nb ? p[lane] : 0.0f;                                // reads stop at n_b
    for (int j = 0; j < nwn; ++j) {
        const bool valid = 64 * j + lane < nb;
        const float v = next;
        if (j + 1 < nwn) next = 64 * (j + 1) + lane < nb ? p[64 * (j + 1) + lane] : 0.0f;   // the next word's load flies over this word's walk
        const unsigned long long H = __ballot(valid && !(v < on));          // NaN counts as speech
        const unsigned long long L = __ballot(valid && v < off);
        const unsigned long long M = ~(H | L), am = H | M;
        const unsigned long long x = H | (M & ((am + H + (unsigned long long)s) ^ am ^ H));   // the 64 states
        s = (int)(x >> 63);                                                 // frames past n_b are MID: the last real frame's state
        const int nbits = nb - 64 * j < 64 ? nb - 64 * j : 64;
        const long long t0 = (long long)m0 + 64 * j;
        int pos = 0;
        while (pos < nbits) {
            const unsigned long long rem = x >> pos;
            const long long tp = t0 + pos;
            long long k;                                                    // boring frames ahead of the next one to look at
            if (mode == EP_IDLE) {
                k = rem ? __builtin_ctzll(rem) : 64;
            } else if (mode == EP_SPEECH) {
                k = ~rem ? __builtin_ctzll(~rem) : 64;
                if (!conf) {
                    const long long kc = lo + min_on - 1 - tp;              // the frame that gives the interval min_on frames
                    k = kc < k ? (kc > 0 ? kc : 0) : k;
                }
            } else {
                k = rem ? __builtin_ctzll(rem) : 64;
                const long long kd = c + D - tp;                            // a zero at frame c + D completes the silence
                k = kd < k ? (kd > 0 ? kd : 0) : k;
                if (!conf && c + poff - lo >= min_on) {
                    const long long kc = lo + min_on - 1 - tp;
                    k = kc < k ? (kc > 0 ? kc : 0) : k;
                }
            }
            if (k >= nbits - pos) break;
            advance(tp + k);
            frame(tp + k, ((rem >> k) & 1ull) != 0);
            pos += (int)k + 1;
        }
    }
    advance(m1);
    const bool end = (fl & UVAD_SLOT_END) != 0;
    if (end) {                                                              // rule 6: n = m1
        if (mode != EP_IDLE && conf) {
            const long long hi = mode == EP_SPEECH ? m1 : (c + poff < m1 ? c + poff : m1);
            emit(2, hi);
            fill(1, hi);
        }
        fill(0, m1);                                                        // an unconfirmed candidate vanishes: zeros from lo on
    }
    const long long nl = F - F0;                                            // 0 .. n_b + lag labels became final
    if (lane == 0) {
        EndpointHystSlot o;
        o.m = end ? 0 : m1;
        o.F = end ? 0 : (int)F;
        o.lo = end ? 0 : (int)lo;
        o.c = end ? 0 : (int)c;
        o.mode = end ? EP_IDLE : mode;
        o.conf = end ? 0 : conf;
        o.s = end ? 0 : s;
        o.reserved = 0;
        *S = o;
        a.ev_counts[b] = nev;
        if (a.active) a.active[b] = (end || mode == EP_IDLE) ? 0 : conf ? 1 : 2;
        if (a.lab_counts) a.lab_counts[b] = (int)nl;
    }
}

}  // namespace

size_t endpoint_hyst_state_bytes(int B) { return sizeof(EndpointHystHeader) + (size_t)B * sizeof(EndpointHystSlot); }

hipError_t launch_endpoint_hyst_reset(void *state, int B, const BinCfgInt &q, hipStream_t s) {
    if (!state || B <= 0) return hipErrorInvalidValue;
    EndpointHystHeader h{};
    h.magic = EPH_MAGIC; h.B = B; h.q = q;
    return launch_state_reset(state, header_words(h), (long long)(endpoint_hyst_state_bytes(B) / sizeof(unsigned)), s);
}

hipError_t launch_endpoint_hyst_step(const EndpointArgs &a, hipStream_t s) {
    if (!a.probs || !a.counts || !a.state || !a.ev_counts || a.B <= 0 || a.ld_in < 1 || a.ld_in > EP_MAX_LD_IN || a.max_events < 0 ||
        (a.labels && (!a.lab_counts || a.ld_lab < a.ld_in)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(endpoint_hyst_step_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
