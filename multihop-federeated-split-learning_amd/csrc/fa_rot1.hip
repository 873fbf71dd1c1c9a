// fa_rot1.hip -- rot1 receipts (fa.h "Rot1 receipts") for CDNA4 (gfx950): an update as one bit per element under a
// randomized Walsh-Hadamard rotation, and one fp32 scale per block of 4096.  Two directions: the expansion of such a
// receipt into an ordinary slot, x = g + D(W(u) scale), and the encoder that makes one from a new model and the model
// the owners hold.
//
// Expansion: a wave per block, on the matrix unit.  W(u) of a vector of +-1 is exact in any order, and H_4096[i][j] =
// (-1)^popcount(i & j) is the Kronecker product of H_16 over any split of the 12 index bits into three groups of four.
// The block is taken as 16 tiles X_t of 16 x 16 with element 256 t + 16 k + m = X_t[m][k]:
//   axis t  register butterflies across the 16 tiles a wave holds, on packed fp16 (values <= 16, exact);
//   axis k  D1 = X_t H with v_mfma_f32_16x16x16_f16: X_t is unpacked from the bits straight into the A layout (lane
//           (r, q) = (lane & 15, lane >> 4) holds X[m = r][k = 4 q + j]), H is a constant built in registers; |D1| <= 256;
//   axis m  D2 = H D1: the D layout of the instruction (lane holds rows 4 q + j of column r) is its B layout, so D1,
//           converted to fp16 (256 is exact), is the second product's B operand as it stands.  |D2| <= 4096, in fp32.
// No transpose is needed: the first operand's layout is free because it is made from bits.  A lane ends with elements
// 256 t + 16 r + 4 q + j, j = 0 .. 3: four consecutive elements per tile, a wave's tile one contiguous run, so a lane moves
// 16 bytes of an fp32 slot (8 of a 16-bit one) per access where the pointers allow it (fa_split.h's rule with V = 4 at
// the bucket's multiples of four) and single elements, each checked against the range, at the ends and elsewhere.
// The signs of D: lanes 0 .. 31 of the wave compute one Philox group (128 elements) each into 512 bytes of LDS, which
// then holds the block's sign mask in the layout of `bits`; a lane reads one word per tile.
//
// Encoder: a workgroup of 256 lanes per block, 16 consecutive elements per lane.  The values are real, so the stages run
// in the rule's order: h = 1 .. 8 in registers, then two LDS transposes (padded by one word per 16: the writes of a lane's
// 16 words and the strided reads hit distinct banks) bring index bits 4 .. 7 and then 8 .. 11 into the registers, and a
// third brings the lane its own 16 elements back.  The lower element of a pair takes a + b and the upper a - b within one
// lane, so a stage is 16 adds per lane.  Then the sign ballot (16 bits per lane, a word per lane pair), the fp64 tree
// (four levels in the lane, xor exchanges in the wave, four wave sums through LDS: fp64 addition commutes, so the
// all-reduce gives the tree's bits), the scale, and for g' the same transform of the signs, exact in fp32.
// Transposes were taken over cross-lane exchanges: 6 x 32 LDS accesses per lane against 2 x (6 x 16 ds_bpermute + 2 x 32
// LDS accesses), which use the same LDS pipe.
//
// Bit-exactness: `#pragma clang fp contract(off)`; the fp32 operations are the subtract of rule 1, the adds of W, the
// decoder's multiply and the expansion's add; the file is compiled without packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "fa_device.h"
#include "fa_host.h"
#include "fa_internal.h"
#include "fa_mx8.h"
#include "fa_philox.h"
#include "fa_rot1.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int64_t kRotMaxBlocks = 4096;  // workgroups per launch; blocks beyond it are strided

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct NoRef {};

__device__ __forceinline__ float rot1_sub(float y, float s) {
#pragma clang fp contract(off)
    return y - s;
}
// ------------------------------------------------------------------ expansion

template <typename T>
__device__ __forceinline__ void load4(const void* p, int64_t e, float* g) {
    if constexpr (sizeof(T) == 4) {
        In<T>::widen(ld16<false>(reinterpret_cast<const T*>(p) + e), g);
    } else {
        const u32x2 v = *reinterpret_cast<const u32x2*>(reinterpret_cast<const T*>(p) + e);
        float w[8];
        In<T>::widen(u32x4{v.x, v.y, 0u, 0u}, w);
        g[0] = w[0]; g[1] = w[1]; g[2] = w[2]; g[3] = w[3];
    }
}

// One wave per block b of the launch (bucket block blk0 + b): see the head of the file.  `first` = the launch's first
// element within its first block (idx0 & 4095); the launch covers elements [0, cnt).
template <typename DST, typename REF>
__global__ __launch_bounds__(kRotThreads) void rot1_expand_kernel(const uint32_t* bits, const float* scale, uint32_t k0,
                                                                  uint32_t k1, uint64_t blk0, int first, int64_t cnt,
                                                                  int64_t nblk, const void* ref, void* dst, int vec) {
    __shared__ __attribute__((aligned(16))) uint32_t sgn[kRotThreads / 64][kRot1Words];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    f16x4 H;  // H_16[r][4 q + j]: the B operand of the first product, the A operand of the second (H is symmetric)
#pragma unroll
    for (int j = 0; j < 4; ++j) H[j] = (__popc(r & (4 * q + j)) & 1) ? (_Float16)-1.0f : (_Float16)1.0f;
    uint32_t* sg = sgn[wave];
    for (int64_t b = (int64_t)blockIdx.x * (kRotThreads / 64) + wave; b < nblk; b += (int64_t)gridDim.x * (kRotThreads / 64)) {
        if (lane < 32) {
            uint32_t w[4];
            rot1_group((blk0 + (uint64_t)b) * 32u + (uint64_t)lane, k0, k1, w);
            *reinterpret_cast<u32x4*>(sg + 4 * lane) = u32x4{w[0], w[1], w[2], w[3]};
        }
        // tile t in the A layout: X_t[m = r][k = 4 q + j] is bit 16 (j & 1) + r of word 8 t + 2 q + (j >> 1)
        const uint32_t* w = bits + b * kRot1Words + 2 * q;
        f16x2 x[16][2];
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                x[t][c] = __builtin_bit_cast(f16x2, 0x3C003C00u | (((w[8 * t + c] >> r) & 0x10001u) << 15));
#pragma unroll
        for (int h = 1; h < 16; h <<= 1)
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (!(t & h)) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const f16x2 a = x[t][c], bb = x[t + h][c];
                        x[t][c] = a + bb;
                        x[t + h][c] = a - bb;
                    }
                }
        const float s = scale[b];
        // the wave's own LDS words: written by lanes 0 .. 31 above, read by every lane below
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int64_t base = b * kRot1Block - first + 16 * r + 4 * q;  // the lane's first element of tile 0 in the launch
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const f16x4 A = f16x4{x[t][0][0], x[t][0][1], x[t][1][0], x[t][1][1]};
            const f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x16f16(A, H, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
            const f16x4 B = f16x4{(_Float16)d1[0], (_Float16)d1[1], (_Float16)d1[2], (_Float16)d1[3]};
            const f32x4 d2 = __builtin_amdgcn_mfma_f32_16x16x16f16(H, B, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
            const int64_t i0 = base + 256 * t;
            if (i0 + 4 <= 0 || i0 >= cnt) continue;
            const uint32_t flips = sg[8 * t + (r >> 1)] >> (16 * (r & 1) + 4 * q);
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = rot1_delta(d2[j], s, (flips >> j) & 1u);
            if (vec && i0 >= 0 && i0 + 4 <= cnt) {
                if constexpr (!__is_same(REF, NoRef)) {
                    float g[4];
                    load4<REF>(ref, i0, g);
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[j] = mx8_add(g[j], d[j]);
                }
                Out<DST>::template store<4, kStPlain>(dst, i0, d);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (i0 + j < 0 || i0 + j >= cnt) continue;
                    float v = d[j];
                    if constexpr (!__is_same(REF, NoRef)) v = mx8_add(In<REF>::scalar(ref, i0 + j), v);
                    Out<DST>::scalar(dst, i0 + j, v);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the next block's signs after this block's reads
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------ encoder

template <typename T>
__global__ __launch_bounds__(kRotThreads) void rot1_encode_kernel(const void* y, const void* sent, int64_t n, int64_t nblk,
                                                                  uint64_t blk0, uint32_t k0, uint32_t k1, uint32_t* bits,
                                                                  float* scale, void* out, int vec) {
    __shared__ float lds[kRotLds];
    __shared__ __attribute__((aligned(16))) uint32_t sgn[kRot1Words];
    __shared__ double wsum[kRotThreads / 64];
    const int tid = threadIdx.x;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int64_t i0 = b * kRot1Block + (int64_t)tid * kRotLane;
        const bool fast = vec && i0 + kRotLane <= n;
        float z[kRotLane], s[kRotLane];
        if (fast) {
            load_ref16<T>(y, i0, z);
            load_ref16<T>(sent, i0, s);
        } else {
#pragma unroll
            for (int e = 0; e < kRotLane; ++e) {
                z[e] = i0 + e < n ? In<T>::scalar(y, i0 + e) : 0.0f;
                s[e] = i0 + e < n ? In<T>::scalar(sent, i0 + e) : 0.0f;
            }
        }
        if (tid < 32) {
            uint32_t w[4];
            rot1_group((blk0 + (uint64_t)b) * 32u + (uint64_t)tid, k0, k1, w);
            *reinterpret_cast<u32x4*>(sgn + 4 * tid) = u32x4{w[0], w[1], w[2], w[3]};
        }
        __syncthreads();
        const uint32_t flips = (sgn[tid >> 1] >> (16 * (tid & 1))) & 0xffffu;  // the lane's 16 signs of D
#pragma unroll
        for (int e = 0; e < kRotLane; ++e)
            z[e] = __uint_as_float(__float_as_uint(rot1_sub(z[e], s[e])) ^ (((flips >> e) & 1u) << 31));
        rot_transform(z, lds);
        uint32_t neg = 0;
        double a[kRotLane];
#pragma unroll
        for (int e = 0; e < kRotLane; ++e) {
            neg |= (z[e] < 0.0f ? 1u : 0u) << e;
            a[e] = (double)__builtin_fabsf(z[e]);
        }
#pragma unroll
        for (int h = 1; h < kRotLane; h <<= 1)
#pragma unroll
            for (int e = 0; e < kRotLane; e += 2 * h) a[e] += a[e + h];
        double wv = a[0];  // tree levels h = 16 .. 512: the lane pairs in ascending distance
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) wv += __shfl_xor(wv, o, 64);
        if ((tid & 63) == 0) wsum[tid >> 6] = wv;
        __syncthreads();
        const double A = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        const bool bad = !(A < (double)INFINITY);  // NaN or +inf
        const float sc = bad ? __uint_as_float(0x7fc00000u) : (float)(A * 0x1p-24);
        if (bad) neg = 0;
        const uint32_t other = (uint32_t)__shfl_xor((int)neg, 1, 64);
        if (!(tid & 1)) bits[b * kRot1Words + (tid >> 1)] = neg | (other << 16);
        if (tid == 0) scale[b] = sc;
        if (out) {  // uniform: g' = sent + D(W(u) scale)
#pragma unroll
            for (int e = 0; e < kRotLane; ++e) z[e] = (neg >> e) & 1u ? -1.0f : 1.0f;
            rot_transform(z, lds);
#pragma unroll
            for (int e = 0; e < kRotLane; ++e) z[e] = mx8_add(s[e], rot1_delta(z[e], sc, (flips >> e) & 1u));
            if (fast) {
                store16<T>(out, i0, z);
            } else {
#pragma unroll
                for (int e = 0; e < kRotLane; ++e)
                    if (i0 + e < n) Out<T>::scalar(out, i0 + e, z[e]);
            }
        }
        __syncthreads();  // wsum and sgn are rewritten by the next block
    }
}

template <typename DST, typename REF>
void launch_expand_t(const uint32_t* bits, const float* scale, uint64_t seed, uint64_t idx0, int64_t cnt, int64_t nblk,
                     const void* ref, void* dst, int vec, hipStream_t s) {
    const int64_t groups = (nblk + kRotThreads / 64 - 1) / (kRotThreads / 64);
    hipLaunchKernelGGL((rot1_expand_kernel<DST, REF>), dim3((unsigned)std::min(groups, kRotMaxBlocks)), dim3(kRotThreads), 0,
                       s, bits, scale, (uint32_t)seed, (uint32_t)(seed >> 32), idx0 >> 12, (int)(idx0 & 4095u), cnt, nblk, ref,
                       dst, vec);
}

template <typename DST>
hipError_t launch_expand_d(const uint32_t* bits, const float* scale, uint64_t seed, uint64_t idx0, int64_t cnt, int64_t nblk,
                           const void* ref, fa_dtype rdt, void* dst, int vec, hipStream_t s) {
    if (!ref) {
        launch_expand_t<DST, NoRef>(bits, scale, seed, idx0, cnt, nblk, ref, dst, vec, s);
    } else if (rdt == FA_F32) {
        launch_expand_t<DST, float>(bits, scale, seed, idx0, cnt, nblk, ref, dst, vec, s);
    } else {  // a 16-bit reference: the slot's own type or an f32 slot (dtype_pair_ok)
        if constexpr (__is_same(DST, float)) {
            if (rdt == FA_BF16) launch_expand_t<DST, uint16_t>(bits, scale, seed, idx0, cnt, nblk, ref, dst, vec, s);
            else launch_expand_t<DST, _Float16>(bits, scale, seed, idx0, cnt, nblk, ref, dst, vec, s);
        } else {
            launch_expand_t<DST, DST>(bits, scale, seed, idx0, cnt, nblk, ref, dst, vec, s);
        }
    }
    return hipGetLastError();
}

template <typename T>
hipError_t launch_encode_t(const void* y, const void* sent, int64_t n, uint64_t blk0, uint64_t seed, uint32_t* bits,
                           float* scale, void* out, int vec, hipStream_t s) {
    const int64_t nblk = (n + kRot1Block - 1) / kRot1Block;
    hipLaunchKernelGGL((rot1_encode_kernel<T>), dim3((unsigned)std::min(nblk, kRotMaxBlocks)), dim3(kRotThreads), 0, s, y,
                       sent, n, nblk, blk0, (uint32_t)seed, (uint32_t)(seed >> 32), bits, scale, out, vec);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rot1_expand(const uint32_t* bits, const float* scale, uint64_t seed, uint64_t idx0, int64_t cnt,
                              const void* ref, fa_dtype rdt, void* dst, fa_dtype ddt, hipStream_t s) {
    if (cnt <= 0) return hipSuccess;
    if (!bits || !scale || !dst || (ref && !dtype_pair_ok(ddt, rdt))) return hipErrorInvalidValue;
    const int64_t nblk = (int64_t)(((idx0 + (uint64_t)cnt - 1) >> 12) - (idx0 >> 12)) + 1;
    // fa_split.h with V = 4: the head brings the launch to the bucket's next multiple of four, where a lane's run starts
    const int64_t lead = (int64_t)((4u - (idx0 & 3u)) & 3u);
    const size_t esd = ddt == FA_F32 ? 4 : 2, esr = rdt == FA_F32 ? 4 : 2;
    Split sp{std::min(lead, cnt), 0, cnt, 4, lead, true};
    sp.vec = sp.after(dst, lead, esd) && (!ref || sp.after(ref, lead, esr));
    switch (ddt) {
        case FA_F32: return launch_expand_d<float>(bits, scale, seed, idx0, cnt, nblk, ref, rdt, dst, sp.vec, s);
        case FA_BF16: return launch_expand_d<uint16_t>(bits, scale, seed, idx0, cnt, nblk, ref, rdt, dst, sp.vec, s);
        case FA_F16: return launch_expand_d<_Float16>(bits, scale, seed, idx0, cnt, nblk, ref, rdt, dst, sp.vec, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_rot1_encode(const void* y, const void* sent, fa_dtype dt, int64_t n, uint64_t blk0, uint64_t seed,
                              uint32_t* bits, float* scale, void* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!y || !sent || !bits || !scale) return hipErrorInvalidValue;
    const size_t es = dt == FA_F32 ? 4 : 2;
    Split sp = split_at(y, es, (size_t)n);  // a lane's 16 elements start at 16 bytes iff the pointers do
    sp.vec = sp.lead == 0;
    sp.require(sent, es);
    if (out) sp.require(out, es);
    switch (dt) {
        case FA_F32: return launch_encode_t<float>(y, sent, n, blk0, seed, bits, scale, out, sp.vec, s);
        case FA_BF16: return launch_encode_t<uint16_t>(y, sent, n, blk0, seed, bits, scale, out, sp.vec, s);
        case FA_F16: return launch_encode_t<_Float16>(y, sent, n, blk0, seed, bits, scale, out, sp.vec, s);
    }
    return hipErrorInvalidValue;
}

void rot1_encode_host(const float* delta, size_t n, uint64_t seed, uint32_t* bits, float* scale) {
    std::vector<float> z(kRot1Block);
    std::vector<double> a(kRot1Block);
    uint32_t sg[kRot1Words];
    for (size_t b = 0; b * kRot1Block < n; ++b) {
        rot1_host_signs(b, seed, sg);
        for (size_t i = 0; i < (size_t)kRot1Block; ++i) {
            const size_t e = b * kRot1Block + i;
            const uint32_t u = e < n ? __builtin_bit_cast(uint32_t, delta[e]) : 0u;
            z[i] = __builtin_bit_cast(float, u ^ ((sg[i >> 5] >> (i & 31) & 1u) << 31));
        }
        rot1_host_transform(z.data());
        for (int i = 0; i < kRot1Block; ++i) a[(size_t)i] = (double)std::fabs(z[(size_t)i]);
        for (int h = 1; h < kRot1Block; h <<= 1)
            for (int i = 0; i < kRot1Block; i += 2 * h) a[(size_t)i] += a[(size_t)(i + h)];
        const bool bad = !(a[0] < (double)INFINITY);
        scale[b] = bad ? __builtin_bit_cast(float, 0x7fc00000u) : (float)(a[0] * 0x1p-24);
        uint32_t* w = bits + b * kRot1Words;
        std::fill(w, w + kRot1Words, 0u);
        for (int i = 0; i < kRot1Block && !bad; ++i)
            if (z[(size_t)i] < 0.0f) w[i >> 5] |= 1u << (i & 31);
    }
}

void rot1_decode_host(const uint32_t* bits, const float* scale, uint64_t seed, uint64_t idx0, size_t cnt, float* d) {
    std::vector<float> v(kRot1Block);
    uint32_t sg[kRot1Words];
    const uint64_t blk0 = idx0 >> 12, end = idx0 + cnt;
    for (uint64_t blk = blk0; blk * kRot1Block < end; ++blk) {
        const uint32_t* w = bits + (blk - blk0) * kRot1Words;
        rot1_host_signs(blk, seed, sg);
        for (int i = 0; i < kRot1Block; ++i) v[(size_t)i] = (w[i >> 5] >> (i & 31) & 1u) ? -1.0f : 1.0f;
        rot1_host_transform(v.data());
        const uint64_t lo = std::max(idx0, blk * kRot1Block), hi = std::min(end, (blk + 1) * kRot1Block);
        for (uint64_t e = lo; e < hi; ++e) {
            const int i = (int)(e & 4095u);
            d[e - idx0] = rot1_delta(v[(size_t)i], scale[blk - blk0], sg[i >> 5] >> (i & 31) & 1u);
        }
    }
}

}  // namespace fa

using namespace fah;

extern "C" {

size_t fa_rot1_blocks(size_t n) { return n / fa::kRot1Block + (n % fa::kRot1Block ? 1 : 0); }
size_t fa_rot1_words(size_t n) { return fa_rot1_blocks(n) * fa::kRot1Words; }

int fa_rot1_encode(const float* delta, size_t n, uint64_t seed, uint32_t* bits, float* scale) {
    g_err.clear();
    if (n == 0) return FA_OK;
    if (!delta || !bits || !scale) return fail(FA_ERR_ARG, "rot1: %s is null", !delta ? "delta" : !bits ? "bits" : "scale");
    fa::rot1_encode_host(delta, n, seed, bits, scale);
    return FA_OK;
}

int fa_rot1_decode(const uint32_t* bits, const float* scale, uint64_t seed, uint64_t idx0, size_t cnt, float* d) {
    g_err.clear();
    if (idx0 + (uint64_t)cnt < idx0) return fail(FA_ERR_ARG, "rot1: idx0 + cnt beyond 2^64");
    if (cnt == 0) return FA_OK;
    if (!bits || !scale || !d) return fail(FA_ERR_ARG, "rot1: %s is null", !bits ? "bits" : !scale ? "scale" : "d");
    fa::rot1_decode_host(bits, scale, seed, idx0, cnt, d);
    return FA_OK;
}

int fa_rot1_expand_device(fa_ctx* ctx, int gpu, const uint32_t* d_bits, const float* d_scale, uint64_t seed, uint64_t idx0,
                          size_t cnt, const void* d_ref, fa_dtype ref_dtype, void* d_dst, fa_dtype dst_dtype,
                          void* hip_stream) {
    g_err.clear();
    // every check before any device call: with cnt == 0 this is the feature probe of a box without a GPU
    if (!dvalid(dst_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (!fa::dtype_pair_ok(dst_dtype, ref_dtype))
        return fail(FA_ERR_ARG, "rot1: no %s slot against a %s reference (a 16-bit slot takes its own type or f32)",
                    fa::dtype_name(dst_dtype), fa::dtype_name(ref_dtype));
    if (idx0 + (uint64_t)cnt < idx0) return fail(FA_ERR_ARG, "rot1: idx0 + cnt beyond 2^64");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (cnt == 0) return FA_OK;
    if (!d_bits || !d_scale || !d_dst)
        return fail(FA_ERR_ARG, "rot1: %s pointer is null", !d_dst ? "d_dst" : !d_bits ? "d_bits" : "d_scale");
    if (!aligned(d_bits, 4) || !aligned(d_scale, 4))
        return fail(FA_ERR_ALIGN, "rot1: %s not 4-byte aligned", !aligned(d_bits, 4) ? "d_bits" : "d_scale");
    if (d_ref && !aligned(d_ref, dsize(ref_dtype)))
        return fail(FA_ERR_ALIGN, "rot1: reference not %zu-byte aligned", dsize(ref_dtype));
    if (!aligned(d_dst, dsize(dst_dtype))) return fail(FA_ERR_ALIGN, "rot1: slot not %zu-byte aligned", dsize(dst_dtype));
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_rot1_expand(d_bits, d_scale, seed, idx0, (int64_t)cnt, d_ref, ref_dtype, d_dst, dst_dtype, c.s));
    return FA_OK;
}

int fa_rot1_encode_device(fa_ctx* ctx, int gpu, const void* d_new, fa_dtype new_dtype, const void* d_sent,
                          fa_dtype sent_dtype, size_t n, uint64_t idx0, uint64_t seed, uint32_t* d_bits, float* d_scale,
                          void* d_out, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!dvalid(new_dtype) || !dvalid(sent_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (new_dtype != sent_dtype)
        return fail(FA_ERR_ARG, "rot1: the new model is %s, the sent one %s: one dtype", fa::dtype_name(new_dtype),
                    fa::dtype_name(sent_dtype));
    if (idx0 % FA_ROT1_BLOCK)
        return fail(FA_ERR_ARG, "rot1: idx0 %llu is no multiple of %d (the encoder takes whole blocks)", (unsigned long long)idx0, FA_ROT1_BLOCK);
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "rot1: idx0 + n beyond 2^64");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if (!d_new || !d_sent || !d_bits || !d_scale)
        return fail(FA_ERR_ARG, "rot1: %s pointer is null", !d_new ? "d_new" : !d_sent ? "d_sent" : !d_bits ? "d_bits" : "d_scale");
    const size_t es = dsize(new_dtype);
    if (!aligned(d_new, es) || !aligned(d_sent, es) || (d_out && !aligned(d_out, es)))
        return fail(FA_ERR_ALIGN, "rot1: %s not %zu-byte aligned", !aligned(d_new, es) ? "d_new" : !aligned(d_sent, es) ? "d_sent" : "d_out", es);
    if (!aligned(d_bits, 4) || !aligned(d_scale, 4))
        return fail(FA_ERR_ALIGN, "rot1: %s not 4-byte aligned", !aligned(d_bits, 4) ? "d_bits" : "d_scale");
    if (d_out) {  // the same address as an input, or apart from it
        const uintptr_t o = (uintptr_t)d_out, bytes = (uintptr_t)(n * es);
        for (const void* in : {d_new, d_sent}) {
            const uintptr_t a = (uintptr_t)in;
            if (o != a && o < a + bytes && a < o + bytes)
                return fail(FA_ERR_ARG, "rot1: d_out overlaps %s without being it", in == d_new ? "d_new" : "d_sent");
        }
    }
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_rot1_encode(d_new, d_sent, new_dtype, (int64_t)n, idx0 >> 12, seed, d_bits, d_scale, d_out, c.s));
    return FA_OK;
}

}  // extern "C"
