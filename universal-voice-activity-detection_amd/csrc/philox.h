// philox.h -- the one counter-based generator of the library: the dropout masks of lstm_train.hip, the noise-mix draws of mix.hip and the
// reverberation draws of reverb.hip
// (include/uvad.h defines every set of coordinates; tests/lstm_dropout_ref.py restates the function).
#pragma once
#include <hip/hip_runtime.h>

namespace uvad {

// Philox4x32-10 (Salmon et al., Random123): ten rounds, the key bumped after each round
__device__ __forceinline__ uint4 lt_philox(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}

}  // namespace uvad
