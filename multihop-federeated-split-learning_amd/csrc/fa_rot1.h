// fa_rot1.h -- what the rot1 codec (fa_rot1.hip) and the rot1-sum stage (fa_rot1_sum.hip) share: the diagonal's Philox
// groups, the decoder's multiply, and the real-valued transform W of a workgroup's block in the rule's fixed order
// (fa.h "Rot1 receipts", Transform W), on the device and on the host.  Every function with fp32 arithmetic carries
// `#pragma clang fp contract(off)`: the rules count roundings.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_internal.h"
#include "fa_philox.h"

namespace fa {

constexpr int kRotThreads = 256, kRotLane = 16;
static_assert(kRot1Block == kRotThreads * kRotLane, "a lane owns 16 elements of its block");
constexpr uint32_t kRotStream = 0x524F5431u;  // counter word 3 of the diagonal: "ROT1"

// Decode rule 3: D applied to fl(v * scale).
__host__ __device__ __forceinline__ float rot1_delta(float v, float scale, uint32_t flip) {
#pragma clang fp contract(off)
    const float d = v * scale;
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, d) ^ (flip << 31));
}

// The sign words of Philox group j (elements 128 j .. 128 j + 127) under the seed's key.
__host__ __device__ __forceinline__ void rot1_group(uint64_t j, uint32_t k0, uint32_t k1, uint32_t* r) {
    philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), 0u, kRotStream, k0, k1, r);
}

constexpr int kRotLds = kRot1Block + kRot1Block / 16;  // one pad word per 16
__device__ __forceinline__ int rot_pad(int i) { return i + (i >> 4); }

// The element of lane T's register e in the three layouts: the lane's own 16 elements; index bits 4 .. 7 in the
// registers; index bits 8 .. 11 in the registers.
enum { kLayOwn = 0, kLayMid = 1, kLayTop = 2 };
template <int L>
__device__ __forceinline__ int rot_elem(int T, int e) {
    if constexpr (L == kLayOwn) return 16 * T + e;
    else if constexpr (L == kLayMid) return 256 * (T >> 4) + 16 * e + (T & 15);
    else return 256 * e + T;
}
template <int FROM, int TO>
__device__ __forceinline__ void rot_exchange(float* z, float* lds) {
    const int T = threadIdx.x;
#pragma unroll
    for (int e = 0; e < kRotLane; ++e) lds[rot_pad(rot_elem<FROM>(T, e))] = z[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kRotLane; ++e) z[e] = lds[rot_pad(rot_elem<TO>(T, e))];
    __syncthreads();
}
// Four stages over the register index, in ascending h: the lower element a + b, the upper a - b.
__device__ __forceinline__ void rot_stages(float* z) {
#pragma clang fp contract(off)
#pragma unroll
    for (int h = 1; h < kRotLane; h <<= 1)
#pragma unroll
        for (int e = 0; e < kRotLane; ++e)
            if (!(e & h)) {
                const float a = z[e], b = z[e + h];
                z[e] = a + b;
                z[e + h] = a - b;
            }
}
// W over the workgroup's block: z in and out as the lane's own 16 elements, h = 1 .. 2048 in the rule's order.
__device__ __forceinline__ void rot_transform(float* z, float* lds) {
    rot_stages(z);
    rot_exchange<kLayOwn, kLayMid>(z, lds);
    rot_stages(z);
    rot_exchange<kLayMid, kLayTop>(z, lds);
    rot_stages(z);
    rot_exchange<kLayTop, kLayOwn>(z, lds);
}

// The host's W and the signs of one block.
inline void rot1_host_transform(float* z) {
#pragma clang fp contract(off)
    for (int h = 1; h < kRot1Block; h <<= 1)
        for (int i = 0; i < kRot1Block; ++i)
            if (!(i & h)) {
                const float a = z[i], b = z[i + h];
                z[i] = a + b;
                z[i + h] = a - b;
            }
}
inline void rot1_host_signs(uint64_t blk, uint64_t seed, uint32_t* sg) {
    for (uint64_t g = 0; g < 32; ++g) rot1_group(blk * 32u + g, (uint32_t)seed, (uint32_t)(seed >> 32), sg + 4 * g);
}

}  // namespace fa
