// Philox4x32-10 (Salmon et al., SC'11): the library's counter-based generator.  c: the 128-bit counter in, four random words out; (k0, k1): the key.
// Used by the Gumbel noise of the hard attention (attention_fused.hip) and by the surface sampler (mesh_metrics.hip).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void rf_philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (unsigned)p1; c[3] = (unsigned)p0; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
