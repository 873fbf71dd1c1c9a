// fa_philox.h -- Philox4x32-10 (Salmon et al., SC 2011), the counter-based generator of the noise stage (fa.h "Noise
// stage", rule 1) and of the diagonal of rot1 receipts (fa.h "Rot1 receipts").  Integer arithmetic only: the same words
// on the host and on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

// Philox4x32-10 of counter (c0..c3) under key (k0, k1).  The 64-bit products are left to the compiler
// (v_mad_u64_u32 on gfx950: one instruction per product).
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                       uint32_t k1, uint32_t* r) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        c1 = (uint32_t)p1;
        c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0;
    r[1] = c1;
    r[2] = c2;
    r[3] = c3;
}

}  // namespace fa
