// fa_mx8.h -- what the MX8 expansion (fa_mx8.hip) and the MX8 encoder (fa_mx8_enc.hip) share: the scale's bit pattern,
// the decoder's two fp32 operations, the scale of a block from its maximum, and 16 elements in 16-byte accesses.
// Every function with fp32 arithmetic carries `#pragma clang fp contract(off)`: the rules count roundings.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_device.h"

namespace fa {

// The fp32 bit pattern of block scale E: 2^(E - 133) for E in 0 .. 254 (biased exponent E - 6 from E = 7 on, below it
// the subnormal with bit E + 16 set), a quiet NaN for 255, which makes every product of the block one.
__host__ __device__ __forceinline__ uint32_t mx8_scale_bits(uint32_t E) {
    return E == 255u ? 0x7fc00000u : E >= 7u ? (E - 6u) << 23 : 1u << (E + 16u);
}
__host__ __device__ __forceinline__ float mx8_scale(uint32_t E) {
    return __builtin_bit_cast(float, mx8_scale_bits(E));
}
// Rule 2: d = fl((float)q * s), one multiply; rule 3: x = fl(g + d), one add.
__host__ __device__ __forceinline__ float mx8_delta(int q, float s) {
#pragma clang fp contract(off)
    return (float)q * s;
}
__host__ __device__ __forceinline__ float mx8_add(float g, float d) {
#pragma clang fp contract(off)
    return g + d;
}

// Encode rules 1-3 on the bit pattern mb of a block's max |delta| (the unsigned maximum of the deltas' bits without
// their signs: a NaN or an inf is above every finite value, so it is the maximum where there is one).  E is the
// smallest scale with m <= 127 * 2^(E - 133), whose pattern is (E << 23) | 0x7E0000 from E = 1 on and the subnormal
// 0x7F0000 at E = 0: the exponent field, one more if the mantissa is beyond 0x7E0000, held at 254.  No frexp.
// Non-decreasing in mb, so the scale of a block is the byte maximum of the scales of its parts.
__host__ __device__ __forceinline__ uint32_t mx8_scale_of_max(uint32_t mb) {
    if (mb >= 0x7f800000u) return 255u;
    if (mb <= 0x007f0000u) return 0u;
    const uint32_t E = (mb >> 23) + ((mb & 0x7fffffu) > 0x7e0000u ? 1u : 0u);
    return E > 254u ? 254u : E;
}
// Encode rule 3's code under scale E: rint(delta 2^(133 - E)) in fp64, where the scaling is exact (2^(133 - E) is an
// fp64 value for every E), ties to even, held to +-127; 0 throughout a block with E = 255.
__host__ __device__ __forceinline__ int mx8_code(float delta, uint32_t E) {
    if (E == 255u) return 0;
    const double up = __builtin_bit_cast(double, (uint64_t)(1023u + 133u - E) << 52);
    double r = __builtin_rint((double)delta * up);
    r = r < -127.0 ? -127.0 : r;
    r = r > 127.0 ? 127.0 : r;
    if (r != r) r = 0.0;  // a NaN under a scale that was given: never in a block the encoder scaled itself
    return (int)r;
}

// 16 elements of T at element e (16-byte aligned there), widened; and 16 results stored as DST.
template <typename T>
__device__ __forceinline__ void load_ref16(const void* ref, int64_t e, float* g) {
    const T* p = reinterpret_cast<const T*>(ref) + e;
#pragma unroll
    for (int j = 0; j < 16; j += In<T>::kVec) In<T>::widen(ld16<false>(p + j), g + j);
}
template <typename DST>
__device__ __forceinline__ void store16(void* dst, int64_t e, const float* x) {
    if constexpr (sizeof(DST) == 4) {
        Out<DST>::template store<16, kStPlain>(dst, e, x);
    } else {
        Out<DST>::template store<8, kStPlain>(dst, e, x);
        Out<DST>::template store<8, kStPlain>(dst, e + 8, x + 8);
    }
}

}  // namespace fa
