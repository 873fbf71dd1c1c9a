// fa_mx8.hip -- MX8 receipts (fa.h "MX8 receipts") for CDNA4 (gfx950): a client's update as int8 codes with one
// power-of-two scale per 32 elements, expanded on the GPU into an ordinary slot, x_i = g_i + q_i 2^(E_b - 133).
//
// Per element the kernel reads 1 byte of q, 1/32 byte of e and 4 or 2 bytes of the reference g, and writes 4 or 2:
// 9 bytes for f32 against f32.  The arithmetic is one conversion, one multiply and one add; no LDS, no cross-lane
// traffic.
//
// Bit-exactness: `#pragma clang fp contract(off)` at file scope and in every function with fp32 arithmetic, as in
// fa_clip.hip: fl(g + fl(q s)) is two roundings and an fma would make it one.  The scale is made from E by
// integer arithmetic on the bit pattern (mx8_scale_bits: a subnormal pattern below E = 7, a quiet NaN for 255), so
// no library function stands between the rule and the bits; the same function serves the host decoder.  It lies in
// fa_mx8.h with the rest that the encoder (fa_mx8_enc.hip) shares.
//
// Two forms by fa::Split (fa_split.h), led by q with one byte per element: a vector is 16 elements.  The vector form
// gives a lane the 16 q bytes at elements head + 16 i .. + 15 in one non-temporal load, the 64 (f32) or 32 (16-bit)
// bytes of g and of the slot in 16-byte accesses.  Those 16 elements are bucket elements G .. G + 15 with
// G = idx0 + head + 16 i: they lie in one block of 32 if G is a multiple of 16 and may straddle two otherwise (a
// pointer phase, or a range that starts off a multiple of 16), so a lane reads the scale of its first and of its last
// element -- neighbours in one cache line -- and element k takes the second from k = 32 - (G & 31) on.  The element
// form takes heads, tails and pointers whose 16-byte phases disagree, one element per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "fa_device.h"
#include "fa_internal.h"
#include "fa_mx8.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

struct NoRef {};  // absolute mode: x = d

// Vector form: lane i of the grid owns vector i, elements head + 16 i .. + 15 of q, ref and dst; g0 = idx0 + head is
// the bucket index of the first of them, b0 = idx0 >> 5 the block e[0] scales.
template <typename DST, typename REF>
__global__ __launch_bounds__(256) void mx8_vec_kernel(const int8_t* q, const uint8_t* e, const void* ref, void* dst,
                                                      int64_t head, int64_t nvec, uint64_t g0, uint64_t b0) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        const int64_t el = head + i * 16;
        const uint64_t g = g0 + (uint64_t)i * 16u;
        const u32x4 w = ld16<true>(q + el);
        const float slo = mx8_scale(e[(g >> 5) - b0]);
        const float shi = mx8_scale(e[((g + 15u) >> 5) - b0]);
        const int kb = 32 - (int)(g & 31u);  // the first k of the next block; > 15: none of this vector
        float x[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int qk = (int)(w[k >> 2] << (24 - 8 * (k & 3))) >> 24;  // byte k & 3, sign-extended
            x[k] = mx8_delta(qk, k < kb ? slo : shi);
        }
        if constexpr (!__is_same(REF, NoRef)) {
            float gr[16];
            load_ref16<REF>(ref, el, gr);
#pragma unroll
            for (int k = 0; k < 16; ++k) x[k] = mx8_add(gr[k], x[k]);
        }
        store16<DST>(dst, el, x);
    }
}

// Element form over elements [0, head) and [tail0, n) (the whole array: head = tail0 = n), one per lane.
template <typename DST, typename REF>
__global__ __launch_bounds__(256) void mx8_elem_kernel(const int8_t* q, const uint8_t* e, const void* ref, void* dst,
                                                       int64_t head, int64_t tail0, int64_t n, uint64_t idx0) {
    const int64_t cnt = head + (n - tail0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t b0 = idx0 >> 5;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cnt; s += stride) {
        const int64_t i = s < head ? s : tail0 + (s - head);
        const uint64_t g = idx0 + (uint64_t)i;
        float x = mx8_delta((int)q[i], mx8_scale(e[(g >> 5) - b0]));
        if constexpr (!__is_same(REF, NoRef)) x = mx8_add(In<REF>::scalar(ref, i), x);
        Out<DST>::scalar(dst, i, x);
    }
}

constexpr int kMx8Block = 256;
constexpr int64_t kMx8MaxBlocks = 1 << 14;  // grid-stride beyond it: 2^22 vectors, a 256 MiB f32 slot, in one trip

unsigned mx8_blocks(int64_t work) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + kMx8Block - 1) / kMx8Block, kMx8MaxBlocks));
}

template <typename DST, typename REF>
hipError_t launch_mx8_t(const int8_t* q, const uint8_t* e, uint64_t idx0, const void* ref, void* dst, const Split& sp,
                        hipStream_t s) {
    if (sp.vec && sp.nvec > 0) {
        hipLaunchKernelGGL((mx8_vec_kernel<DST, REF>), dim3(mx8_blocks(sp.nvec)), dim3(kMx8Block), 0, s, q, e, ref, dst,
                           sp.head, sp.nvec, idx0 + (uint64_t)sp.head, idx0 >> 5);
        if (sp.edges() > 0)
            hipLaunchKernelGGL((mx8_elem_kernel<DST, REF>), dim3(1), dim3(64), 0, s, q, e, ref, dst, sp.head, sp.tail0(),
                               sp.n, idx0);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((mx8_elem_kernel<DST, REF>), dim3(mx8_blocks(sp.n)), dim3(kMx8Block), 0, s, q, e, ref, dst, sp.n,
                       sp.n, sp.n, idx0);
    return hipGetLastError();
}

template <typename DST>
hipError_t launch_mx8_d(const int8_t* q, const uint8_t* e, uint64_t idx0, const void* ref, fa_dtype rdt, void* dst,
                        const Split& sp, hipStream_t s) {
    if (!ref) return launch_mx8_t<DST, NoRef>(q, e, idx0, ref, dst, sp, s);
    switch (rdt) {
        case FA_F32: return launch_mx8_t<DST, float>(q, e, idx0, ref, dst, sp, s);
        case FA_BF16:
            if constexpr (!__is_same(DST, _Float16)) return launch_mx8_t<DST, uint16_t>(q, e, idx0, ref, dst, sp, s);
            break;
        case FA_F16:
            if constexpr (!__is_same(DST, uint16_t)) return launch_mx8_t<DST, _Float16>(q, e, idx0, ref, dst, sp, s);
            break;
    }
    return hipErrorInvalidValue;
}

}  // namespace

// The split of one expansion: led by q (one byte per element, 16 per vector), the slot and the reference required
// after the same head.  A common head exists only if the three 16-byte phases agree: (q + h) = 0, (dst + h sd) = 0 and
// (ref + h sr) = 0 mod 16 for one h -- Split::require is that test.
Split mx8_split(const void* q, size_t n, const void* ref, fa_dtype rdt, const void* dst, fa_dtype ddt) {
    Split sp = split_at(q, 1, n);
    sp.require(dst, ddt == FA_F32 ? 4 : 2);
    if (ref) sp.require(ref, rdt == FA_F32 ? 4 : 2);
    return sp;
}

hipError_t launch_mx8_expand(const int8_t* q, const uint8_t* e, uint64_t idx0, int64_t n, const void* ref, fa_dtype rdt,
                             void* dst, fa_dtype ddt, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!q || !e || !dst || (ref && !dtype_pair_ok(ddt, rdt))) return hipErrorInvalidValue;
    const Split sp = mx8_split(q, (size_t)n, ref, rdt, dst, ddt);
    if (!sp.valid()) return hipErrorInvalidValue;
    switch (ddt) {
        case FA_F32: return launch_mx8_d<float>(q, e, idx0, ref, rdt, dst, sp, s);
        case FA_BF16: return launch_mx8_d<uint16_t>(q, e, idx0, ref, rdt, dst, sp, s);
        case FA_F16: return launch_mx8_d<_Float16>(q, e, idx0, ref, rdt, dst, sp, s);
    }
    return hipErrorInvalidValue;
}

void mx8_decode_host(const int8_t* q, const uint8_t* e, size_t n, uint64_t idx0, float* d) {
    const uint64_t b0 = idx0 >> 5;
    for (size_t i = 0; i < n; ++i) d[i] = mx8_delta((int)q[i], mx8_scale(e[((idx0 + i) >> 5) - b0]));
}

void mx8_encode_host(const float* delta, size_t n, int8_t* q, uint8_t* e) {
    for (size_t lo = 0, b = 0; lo < n; lo += FA_MX8_BLOCK, ++b) {
        const size_t hi = std::min(n, lo + (size_t)FA_MX8_BLOCK);
        bool finite = true;
        float m = 0.0f;
        for (size_t i = lo; i < hi; ++i) {
            const float a = std::fabs(delta[i]);
            if (!(a <= 3.402823466e+38f)) finite = false;  // NaN or inf
            else if (a > m) m = a;
        }
        if (!finite || m == 0.0f) {
            e[b] = finite ? 0 : 255;
            for (size_t i = lo; i < hi; ++i) q[i] = 0;
            continue;
        }
        int k;
        const float f = std::frexp(m, &k);  // m = f 2^k, f in [0.5, 1)
        int t = f <= 127.0f / 128.0f ? k - 7 : k - 6;  // the smallest t with m 2^-t <= 127
        const int E = std::min(std::max(t + 133, 0), 254);
        t = E - 133;
        e[b] = (uint8_t)E;
        for (size_t i = lo; i < hi; ++i) {
            const double r = std::rint(std::ldexp((double)delta[i], -t));  // exact scaling, ties to even
            q[i] = (int8_t)std::min(std::max(r, -127.0), 127.0);
        }
    }
}

}  // namespace fa
