// fa_sortnet.h -- what the per-element sorting kernels share (fa_trimmed.hip, fa_centered.hip): the keys of the
// FA_TRIMMED total order (fa.h), the compare-exchange, the bitonic network over a register array, the load
// guard of a padded width and the grid sizing.  Device code, included by those two files only.
#ifndef FA_SORTNET_H_
#define FA_SORTNET_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_internal.h"

namespace fa {

namespace {

// k(x) of fa.h: NaN -> 0xFFFFFFFF, sign set -> ~bits, else bits | 0x80000000.
__device__ __forceinline__ uint32_t trim_key(float x) {
    const uint32_t b = __float_as_uint(x);
    const uint32_t k = b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
    return (b & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : k;
}
// Its inverse; 0xFFFFFFFF decodes to the quiet NaN 0x7FFFFFFF.
__device__ __forceinline__ float trim_value(uint32_t k) {
    return __uint_as_float(k ^ (~(uint32_t)((int32_t)k >> 31) | 0x80000000u));
}

__device__ __forceinline__ void cmp_exchange(uint32_t& lo, uint32_t& hi) {
    const uint32_t a = lo < hi ? lo : hi;
    hi = lo < hi ? hi : lo;
    lo = a;
}

// Bitonic sorting network in its all-ascending form: the merge of width w first compares i with its mirror
// i ^ (w - 1), then halves (i with i ^ j).  P log2(P) (log2(P) + 1) / 4 compare-exchanges: 672 at P = 64.
template <int P>
__device__ __forceinline__ void sort_keys(uint32_t (&k)[P]) {
    // loops over the exponents (w = 2^lw, j = 2^lj): linear trip counts, so every one of them unrolls
#pragma unroll
    for (int lw = 1; (1 << lw) <= P; ++lw) {
        const int w = 1 << lw;
#pragma unroll
        for (int i = 0; i < P; ++i)
            if ((i ^ (w - 1)) > i) cmp_exchange(k[i], k[i ^ (w - 1)]);
#pragma unroll
        for (int lj = lw - 2; lj >= 0; --lj) {
            const int j = 1 << lj;
#pragma unroll
            for (int i = 0; i < P; ++i)
                if ((i ^ j) > i) cmp_exchange(k[i], k[i ^ j]);
        }
    }
}

// Clients per launch are P/2 < nc <= P (nc = 1 takes P = 2), so the first half of the loads needs no guard.
template <int P>
__device__ __forceinline__ bool client_live(int u, int nc) { return u < (P + 1) / 2 || u < nc; }

constexpr int kWideBlock = 64;               // the wide forms (64 < nc <= 128): one wave per block
constexpr int64_t kElemMaxBlocks = 1 << 16;  // grid-stride beyond it
inline int64_t blocks_for(int64_t work, const Tuning& tu, int64_t cap) {
    int64_t g = (work + tu.block - 1) / tu.block;
    if (tu.max_blocks > 0) cap = std::min<int64_t>(cap, tu.max_blocks);
    return std::max<int64_t>(1, std::min(g, cap));
}

}  // namespace

}  // namespace fa

#endif  // FA_SORTNET_H_
