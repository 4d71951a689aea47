// state_reset.hip -- the reset of every device state that is a 256-byte header followed by slots that start as zeros: the live endpointers
// (endpoint.hip, endpoint_hyst.hip) and the live speech gates (gate.hip, gate_group.hip).  Their launchers fill the header struct by field
// name and call launch_state_reset with its 64 words (header_words, uvad_internal.h) and the word count of header plus slots.
//   state_reset_kernel   state[i] = i < 64 ? word i of the header : 0, a grid-stride loop; the header comes in the kernel's arguments
#include "uvad_internal.h"

namespace uvad {

namespace {

__global__ __launch_bounds__(256) void state_reset_kernel(unsigned *state, HeaderWords h, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) state[i] = i < 64 ? h.w[i] : 0u;
}

}  // namespace

hipError_t launch_state_reset(void *state, const HeaderWords &h, long long n_words, hipStream_t s) {
    if (!state || n_words < 64) return hipErrorInvalidValue;
    const long long g = (n_words + 255) / 256;
    hipLaunchKernelGGL(state_reset_kernel, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(256), 0, s, reinterpret_cast<unsigned *>(state), h, n_words);
    return hipGetLastError();
}

}  // namespace uvad
