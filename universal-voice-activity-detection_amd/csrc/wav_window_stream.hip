// wav_window_stream.hip -- the PCM ring and window assembly of the waveform model's windowed stream (uvad_window_wav_step,
// include/uvad.h).
//
// SincNet normalises every stage over the whole row, so the stream keeps the raw samples, not features: per feed a ring of ring_len
// samples in the state (sample p in slot p % ring_len), in the state's sample type (f32, or int16 read as q / 32768 by the SincNet
// stages).  Each step wav_window_assemble_kernel
//   * reads n_prev (samples received before the step) from the DEVICE counter *ctr_in, so that a graph captured around one
//     steady-state step replays correctly for any later one with the same launch arguments,
//   * commits the step's chunk to slots [n_prev, n_prev + chunk),
//   * writes the window of Tw frames -- samples [J (e - Tw), J (e - Tw) + Sw), e = frames(n) complete frames -- contiguously to out
//     [B][Sw], the chunk's samples from the chunk and older ones from the ring, so that the unchanged SincNet stages read a plain
//     (B, Sw) batch,
//   * and stores n in *ctr_out for the next step.
// The window ends at J (e - 1) + R <= n and starts less than Sw + J samples before n; with ring_len >= Sw_max + J the ring slots it
// reads ([start, n_prev)) and the ones the chunk writes ([n_prev, n)) differ, so no thread reads a slot another one writes.
// Global memory only: no LDS, no scratch (tests/test_abi_wav_window_stream.py reads the ISA).
#include "uvad_internal.h"

namespace uvad {

namespace {

template <typename T>
__global__ __launch_bounds__(256) void wav_window_assemble_kernel(WavWindowArgs a) {
    const int b = blockIdx.y;
    const long long n_prev = a.ctr_in[0], n = n_prev + a.chunk_len;
    if (a.ctr_out && b == 0 && blockIdx.x == 0 && threadIdx.x == 0) a.ctr_out[0] = n;
    const long long e = n < a.R ? 0 : (n - a.R) / a.J + 1;
    const long long lo = e >= a.Tw ? (long long)a.J * (e - a.Tw) : 0;   // (e < Tw only if the host and device counters disagree)
    const long long cbase = n_prev % a.ring_len, wbase = lo % a.ring_len;
    const T *chunk = static_cast<const T *>(a.chunk) + (size_t)b * a.chunk_len;
    T *ring = static_cast<T *>(a.ring) + (size_t)b * a.ring_len;
    T *out = a.out ? static_cast<T *>(a.out) + (size_t)b * a.Sw : nullptr;
    const int items = a.chunk_len + (out ? a.Sw : 0);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += gridDim.x * blockDim.x) {
        if (i < a.chunk_len) {
            long long slot = cbase + i;
            if (slot >= a.ring_len) slot -= a.ring_len;
            ring[slot] = chunk[i];
            continue;
        }
        const int j = i - a.chunk_len;
        const long long p = lo + j;   // absolute sample index
        T v = T(0);
        if (p >= n_prev) {
            if (p < n) v = chunk[p - n_prev];
        } else {
            long long slot = wbase + j;
            if (slot >= a.ring_len) slot -= a.ring_len;
            v = ring[slot];
        }
        out[j] = v;
    }
}

}  // namespace

hipError_t launch_wav_window_assemble(const WavWindowArgs &a, int is_i16, hipStream_t s) {
    if (!a.chunk || !a.ring || !a.ctr_in || a.B <= 0 || a.B > 65535 || a.chunk_len <= 0 || a.J <= 0 || a.R <= 0 || a.Tw < 0)
        return hipErrorInvalidValue;
    if (a.out && (a.Tw < 1 || a.Sw != a.R + a.J * (a.Tw - 1))) return hipErrorInvalidValue;
    // every slot one launch touches is distinct: the chunk plus the window's reach back from n
    if (a.ring_len < a.chunk_len || (a.out && a.ring_len < (long long)a.Sw + a.J)) return hipErrorInvalidValue;
    const long long items = (long long)a.chunk_len + (a.out ? a.Sw : 0);
    if (items > 0x7fffffffLL) return hipErrorInvalidValue;
    const long long want = (items + 255) / 256, cap = 4 + 4096 / a.B;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)a.B);
    if (is_i16) hipLaunchKernelGGL(wav_window_assemble_kernel<int16_t>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(wav_window_assemble_kernel<float>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace uvad
