// fa_rot1_sum.hip -- the rot1-sum stage (fa.h "Rot1-sum stage") for CDNA4 (gfx950): the rot1 receipts of a round
// reduced in the rotated domain, without expanding a receipt into a dense slot.  The transform is linear, so for the
// owners that share a seed s
//     sum_c w_c D_s(scale_c W u_c) = D_s W(sum_c (w_c scale_c) u_c):
// per rotated coordinate the owners' signed scalars are added, D adds and no multiply, then one real-valued transform per
// block and seed runs, and g is added once.  Per element that is D / 8 bytes of bits, g once and the output once, where
// fa_submit_rot1 and the chain move about 12 D + 4.
//
// A workgroup of 256 lanes owns a block of 4096 elements and a lane 16 consecutive ones, the encoder's "own" layout: the
// lane's 16 bits of an owner are one half-word, a wave's 64 half-words 128 contiguous bytes.  Blocks are dealt over a
// grid of what is co-resident, the rest strided.
//   Accumulation, per seed group: 16 accumulators z in registers.  Per owner one block-uniform t = fl(w * scale)
//   (the weight, the scale pointer and the scale itself are scalar loads; one v_mul per owner) and one 2-byte load of
//   the lane's half-word.  The sign of t is folded into the half-word once per owner (one xor with t >> 31), so an
//   element costs a shift, a bit-field insert of the bit into t, and the add: 3 VALU operations (the compiled ISA has 51
//   per owner and 16 elements: 16 v_lshlrev_b32, 16 v_bfi_b32, 16 v_add_f32 and the v_mul, the v_ashrrev and the v_xor of
//   the fold; the hand-over and the table's SGPRs kept in VGPR lanes add about 5 per owner).
//   Loads in flight: the half-words, scales and weights of the next kRot1SumDepth = 8 owners are loaded before the
//   current 8 are applied -- the next owners of the group, else the first of the next group, else those of the
//   workgroup's next block, so the transform and the output run under loads as well.  One owner's block is 512 bytes, 8
//   bytes per wave and owner in a 128-byte line: a round trip per owner would be latency-bound.  The fetch is
//   straight-line code (every one of the 8 loads is issued, the ones beyond the group on its last owner again) and the
//   registers are handed over at one place, so the ISA waits for loads only there (vmcnt(0) once per 8 owners) and the 8
//   x 51 VALU operations of 4 cycles, about 1600 cycles, run under the next loads; 4 waves per SIMD cover the rest.  A
//   depth of 16 would cost 32 more VGPRs for loads that 8 owners' work already covers.
//   Per group then: rot_transform (12 stages, three padded LDS transposes, fa_rot1.h), the Philox signs of the group's
//   seed through 512 bytes of LDS as the encoder does (lanes 0 .. 31 compute a Philox group each; two buffers taken in
//   turn, so that the next group's signs need no barrier of their own: between a buffer's reads and its next writes lie
//   the barriers of a whole transform), the sign flip and the add into 16 acc registers.
//   Output: g in 16-byte loads, one add, 16-byte stores where both pointers are 16-byte aligned at the bucket's
//   multiples of 16 (`vec`); lanes that straddle the launch's range, and every lane for other phases, go element by
//   element, each store checked against the range.  The arithmetic is the same, so the bits do not depend on it.
//
// The owner table -- bits, scale, seed and w of up to 128 owners in the order of rule 0 and one bit per owner that
// starts a group, 3600 bytes -- travels in the kernel-argument segment (4 KiB) as arrays of 8-byte and 4-byte entries,
// each array 8-byte aligned: every access to it is a dword-aligned scalar load with a wave-uniform index.
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950): 110 - 111 VGPRs in every dtype pair, 0 AGPRs, 106 SGPRs
// (56 more kept in VGPR lanes, no memory), 18432 bytes of LDS (17408 for the transposes, 2 x 512 for the signs), no
// scratch, 4 waves per SIMD -- 4 workgroups per CU, which is the grid's cap.  Measured: 0.048 - 0.132 of
// the expanded route's device time with one seed, 0.41 - 0.42 with a seed per owner.
//
// Bit-exactness: `#pragma clang fp contract(off)`.  The fp32 operations are the multiply of rule 1, the adds of rules 2,
// 5 and 6 and the adds and subtracts of W; the file is compiled without packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "fa_device.h"
#include "fa_host.h"
#include "fa_internal.h"
#include "fa_mx8.h"
#include "fa_rot1.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kDepth = kRot1SumDepth;  // the owners whose half-words and scales are in flight
constexpr int64_t kMaxGrid = 256 * 4;  // 256 CUs x the workgroups co-resident on one; blocks beyond it are strided

struct NoRef {};

struct Rot1SumTable {  // 3600 bytes of the kernel-argument segment, in the order of rule 0
    const uint32_t* bits[kMaxClients];
    const float* scale[kMaxClients];
    uint64_t seed[kMaxClients];
    float w[kMaxClients];
    uint32_t first[kMaxClients / 32];  // bit c: owner c starts a group
};
static_assert(sizeof(Rot1SumTable) == 3600, "the table and the rest of the arguments fit in 4 KiB");

// One launch: cnt elements from element `first` of bucket block blk0 on, nblk blocks.
struct Rot1SumLanes {
    int64_t cnt, nblk;
    uint64_t blk0;
    int first, D, vec;
};

__host__ __device__ __forceinline__ float sum_mul(float w, float s) {
#pragma clang fp contract(off)
    return w * s;
}
__host__ __device__ __forceinline__ float sum_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// The end of the group that starts at owner c: the next owner that starts one, or D.
__device__ __forceinline__ int group_end(const Rot1SumTable& tb, int c, int D) {
    for (++c; c < D;) {
        const uint32_t m = tb.first[c >> 5] >> (c & 31);
        if (m) return std::min(c + (int)__builtin_ctz(m), D);
        c = (c | 31) + 1;
    }
    return D;
}

// (keep & t) | (~keep & sh): the sign from sh, the rest from t.  Written as the instruction: from the C expression the
// compiler forms v_and_b32 and v_or_b32 (a VOP3 instruction takes no literal mask), four operations per element for three.
__device__ __forceinline__ uint32_t sign_insert(uint32_t keep, uint32_t t, uint32_t sh) {
    uint32_t d;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "s"(keep), "v"(t), "v"(sh));
    return d;
}

// Rules 1-2 for one owner on a lane's 16 positions: its half-word hw, its scale sc, its weight w; keep = 0x7fffffff.
__device__ __forceinline__ void apply16(uint32_t hw, float sc, float w, uint32_t keep, float* z) {
    const uint32_t t = __float_as_uint(sum_mul(w, sc));
    const uint32_t x = hw ^ (uint32_t)((int32_t)t >> 31);  // bit e: the sign of s at position e
#pragma unroll
    for (int e = 0; e < kRotLane; ++e) z[e] = sum_add(z[e], __uint_as_float(sign_insert(keep, t, x << (31 - e))));
}

template <typename DST, typename REF>
__global__ __launch_bounds__(kRotThreads) void rot1sum_kernel(const Rot1SumTable tb, const Rot1SumLanes ln, const void* ref,
                                                              void* dst) {
    __shared__ float lds[kRotLds];
    __shared__ __attribute__((aligned(16))) uint32_t sgn[2][kRot1Words];
    const int tid = (int)threadIdx.x, D = ln.D;
    const int ge0 = group_end(tb, 0, D);
    const uint32_t keep = 0x7fffffffu;
    // owners [c0, ce) of block bb, c0 < ce, at most kDepth: the lane's half-words, the block's scales, the weights.
    // Every one of the kDepth loads is issued, those beyond ce on owner ce - 1 again: straight-line code, so the
    // compiler counts the loads in flight and waits for the current owners' only, not for the next ones' as well.
    const auto fetch = [&](int64_t bb, int c0, int ce, uint32_t* hw, float* sc, float* ww) {
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            const int c = std::min(c0 + u, ce - 1);
            hw[u] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(tb.bits[c]) + bb * (2 * kRot1Words) + tid);
            sc[u] = tb.scale[c][bb];
            ww[u] = tb.w[c];
        }
    };
    uint32_t cur[kDepth], nxt[kDepth];
    float scur[kDepth], snxt[kDepth], wcur[kDepth], wnxt[kDepth];
    if ((int64_t)blockIdx.x < ln.nblk) fetch(blockIdx.x, 0, ge0, nxt, snxt, wnxt);
    // vmcnt(0) here, once: the compiler then knows at the loop's head that only the loads issued in it are in flight
    __builtin_amdgcn_s_waitcnt(0x0F70);
    int par = 0;
    for (int64_t b = blockIdx.x; b < ln.nblk; b += gridDim.x) {
        float acc[kRotLane];
#pragma unroll
        for (int e = 0; e < kRotLane; ++e) acc[e] = 0.0f;
        for (int gs = 0, ge = ge0; gs < D;) {
            const int gn = ge < D ? group_end(tb, ge, D) : D;  // the end of the next group
            float z[kRotLane];
#pragma unroll
            for (int e = 0; e < kRotLane; ++e) z[e] = 0.0f;
            for (int c0 = gs; c0 < ge; c0 += kDepth) {
#pragma unroll
                for (int u = 0; u < kDepth; ++u) {  // what was in flight: the one place that waits for loads
                    cur[u] = nxt[u];
                    scur[u] = snxt[u];
                    wcur[u] = wnxt[u];
                }
                // the next owners of the group, else the first of the next group, else of the workgroup's next block
                // (after the last block: the first again, which nobody uses)
                if (c0 + kDepth < ge) fetch(b, c0 + kDepth, ge, nxt, snxt, wnxt);
                else if (ge < D) fetch(b, ge, gn, nxt, snxt, wnxt);
                else fetch(b + gridDim.x < ln.nblk ? b + gridDim.x : b, 0, ge0, nxt, snxt, wnxt);
#pragma unroll
                for (int u = 0; u < kDepth; ++u)
                    if (c0 + u < ge) apply16(cur[u], scur[u], wcur[u], keep, z);
            }
            if (tid < 32) {
                uint32_t w[4];
                const uint64_t seed = tb.seed[gs];
                rot1_group((ln.blk0 + (uint64_t)b) * 32u + (uint64_t)tid, (uint32_t)seed, (uint32_t)(seed >> 32), w);
                *reinterpret_cast<u32x4*>(&sgn[par][4 * tid]) = u32x4{w[0], w[1], w[2], w[3]};
            }
            rot_transform(z, lds);  // its barriers order the signs' writes before the reads below
            const uint32_t flips = sgn[par][tid >> 1] >> (16 * (tid & 1));  // the lane's 16 signs of D
#pragma unroll
            for (int e = 0; e < kRotLane; ++e)
                acc[e] = sum_add(acc[e], __uint_as_float(__float_as_uint(z[e]) ^ (((flips >> e) & 1u) << 31)));
            par ^= 1;
            gs = ge;
            ge = gn;
        }
        const int64_t el = b * kRot1Block - ln.first + (int64_t)tid * kRotLane;  // the lane's first element in the launch
        if (el + kRotLane <= 0 || el >= ln.cnt) continue;
        if (ln.vec && el >= 0 && el + kRotLane <= ln.cnt) {
            if constexpr (!__is_same(REF, NoRef)) {
                float g[kRotLane];
                load_ref16<REF>(ref, el, g);
#pragma unroll
                for (int e = 0; e < kRotLane; ++e) acc[e] = sum_add(g[e], acc[e]);
            }
            store16<DST>(dst, el, acc);
        } else {
#pragma unroll
            for (int e = 0; e < kRotLane; ++e) {
                if (el + e < 0 || el + e >= ln.cnt) continue;
                float v = acc[e];
                if constexpr (!__is_same(REF, NoRef)) v = sum_add(In<REF>::scalar(ref, el + e), v);
                Out<DST>::scalar(dst, el + e, v);
            }
        }
    }
}

template <typename DST, typename REF>
void launch_t(const Rot1SumTable& tb, const Rot1SumLanes& ln, const void* ref, void* dst, int64_t cap, hipStream_t s) {
    hipLaunchKernelGGL((rot1sum_kernel<DST, REF>), dim3((unsigned)std::min(ln.nblk, cap)), dim3(kRotThreads), 0, s, tb, ln,
                       ref, dst);
}

template <typename DST>
void launch_d(const Rot1SumTable& tb, const Rot1SumLanes& ln, const void* ref, fa_dtype rdt, void* dst, int64_t cap,
              hipStream_t s) {
    if (!ref) {
        launch_t<DST, NoRef>(tb, ln, ref, dst, cap, s);
    } else if (rdt == FA_F32) {
        launch_t<DST, float>(tb, ln, ref, dst, cap, s);
    } else {  // a 16-bit reference: the output's own type or an f32 output (dtype_pair_ok)
        if constexpr (__is_same(DST, float)) {
            if (rdt == FA_BF16) launch_t<DST, uint16_t>(tb, ln, ref, dst, cap, s);
            else launch_t<DST, _Float16>(tb, ln, ref, dst, cap, s);
        } else {
            launch_t<DST, DST>(tb, ln, ref, dst, cap, s);
        }
    }
}

}  // namespace

// Rule 0: order[k] is the owner at place k, the groups by their lowest slot and within a group ascending; first[k] says
// that place k starts a group.
void rot1_sum_order(const uint64_t* seed, int D, int* order, uint8_t* first) {
    std::vector<char> used((size_t)D, 0);
    int k = 0;
    for (int c = 0; c < D; ++c) {
        if (used[(size_t)c]) continue;
        for (int o = c; o < D; ++o)
            if (!used[(size_t)o] && seed[o] == seed[c]) {
                used[(size_t)o] = 1;
                first[k] = o == c;
                order[k++] = o;
            }
    }
}

// Whether a lane's 16 elements may move in 16-byte accesses: p is 16-byte aligned at the bucket's multiples of 16.
bool rot1_sum_vec(uint64_t idx0, const void* ref, fa_dtype rdt, const void* out, fa_dtype odt) {
    const auto ok = [idx0](const void* p, fa_dtype dt) {
        return ((uintptr_t)p - (uintptr_t)(idx0 & 15u) * (dt == FA_F32 ? 4u : 2u)) % 16 == 0;
    };
    return ok(out, odt) && (!ref || ok(ref, rdt));
}

hipError_t launch_rot1_sum(const uint32_t* const* bits, const float* const* scale, const uint64_t* seed, const float* w, int D,
                           uint64_t idx0, int64_t cnt, const void* ref, fa_dtype rdt, void* out, fa_dtype odt, const Tuning& tu,
                           hipStream_t s) {
    if (cnt <= 0) return hipSuccess;
    if (D < 1 || D > kMaxClients || !bits || !scale || !seed || !w || !out || (ref && !dtype_pair_ok(rdt, odt)))
        return hipErrorInvalidValue;
    int order[kMaxClients];
    uint8_t first[kMaxClients];
    rot1_sum_order(seed, D, order, first);
    Rot1SumTable tb{};
    for (int k = 0; k < D; ++k) {
        const int c = order[k];
        if (!bits[c] || !scale[c]) return hipErrorInvalidValue;
        tb.bits[k] = bits[c];
        tb.scale[k] = scale[c];
        tb.seed[k] = seed[c];
        tb.w[k] = w[c];
        if (first[k]) tb.first[k >> 5] |= 1u << (k & 31);
    }
    const int64_t nblk = (int64_t)(((idx0 + (uint64_t)cnt - 1) >> 12) - (idx0 >> 12)) + 1;
    const Rot1SumLanes ln{cnt, nblk, idx0 >> 12, (int)(idx0 & 4095u), D, rot1_sum_vec(idx0, ref, rdt, out, odt) ? 1 : 0};
    int64_t cap = kMaxGrid;
    if (tu.max_blocks > 0) cap = std::min<int64_t>(cap, tu.max_blocks);
    switch (odt) {
        case FA_F32: launch_d<float>(tb, ln, ref, rdt, out, cap, s); break;
        case FA_BF16: launch_d<uint16_t>(tb, ln, ref, rdt, out, cap, s); break;
        case FA_F16: launch_d<_Float16>(tb, ln, ref, rdt, out, cap, s); break;
    }
    return hipGetLastError();
}

// Rules 0-6 on the host, block by block: per group the chain over its owners at all 4096 positions, W, D, the sum over
// the groups, then the reference inside the range.
void rot1_sum_host(const uint32_t* const* bits, const float* const* scale, const uint64_t* seed, const float* w, int D,
                   uint64_t idx0, size_t cnt, const float* ref, float* out) {
#pragma clang fp contract(off)
    std::vector<int> order((size_t)D);
    std::vector<uint8_t> first((size_t)D);
    rot1_sum_order(seed, D, order.data(), first.data());
    std::vector<float> z(kRot1Block), acc(kRot1Block);
    uint32_t sg[kRot1Words];
    const uint64_t blk0 = idx0 >> 12, end = idx0 + cnt;
    for (uint64_t blk = blk0; blk * kRot1Block < end; ++blk) {
        std::fill(acc.begin(), acc.end(), 0.0f);
        for (int k = 0; k < D;) {
            const uint64_t sd = seed[order[(size_t)k]];
            std::fill(z.begin(), z.end(), 0.0f);
            do {
                const int c = order[(size_t)k];
                const uint32_t t = __builtin_bit_cast(uint32_t, sum_mul(w[c], scale[c][blk - blk0]));
                const uint32_t* wd = bits[c] + (blk - blk0) * kRot1Words;
                for (int j = 0; j < kRot1Block; ++j)
                    z[(size_t)j] = sum_add(z[(size_t)j], __builtin_bit_cast(float, t ^ ((wd[j >> 5] >> (j & 31) & 1u) << 31)));
            } while (++k < D && !first[(size_t)k]);
            rot1_host_transform(z.data());
            rot1_host_signs(blk, sd, sg);
            for (int i = 0; i < kRot1Block; ++i) {
                const uint32_t v = __builtin_bit_cast(uint32_t, z[(size_t)i]) ^ ((sg[i >> 5] >> (i & 31) & 1u) << 31);
                acc[(size_t)i] = sum_add(acc[(size_t)i], __builtin_bit_cast(float, v));
            }
        }
        const uint64_t lo = std::max(idx0, blk * kRot1Block), hi = std::min(end, (blk + 1) * kRot1Block);
        for (uint64_t e = lo; e < hi; ++e) {
            const float a = acc[(size_t)(e & 4095u)];
            out[e - idx0] = ref ? sum_add(ref[e - idx0], a) : a;
        }
    }
}

}  // namespace fa

using namespace fah;

namespace {

// What fa_rot1_sum_host and fa_rot1_sum_device refuse before they look at a pointer's target.
int check_rot1_sum(const void* const* bits, const void* const* scale, const uint64_t* seed, const float* w, int D, size_t cnt,
                   uint64_t idx0) {
    if (D < 1 || D > FA_ROT1_SUM_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "rot1 sum: D = %d clients outside 1 .. %d", D, FA_ROT1_SUM_MAX_CLIENTS);
    if (idx0 + (uint64_t)cnt < idx0) return fail(FA_ERR_ARG, "rot1 sum: idx0 + cnt beyond 2^64");
    if (cnt == 0) return FA_OK;
    if (!bits || !scale || !seed || !w)
        return fail(FA_ERR_ARG, "rot1 sum: %s is null", !bits ? "bits" : !scale ? "scale" : !seed ? "seed" : "w");
    for (int c = 0; c < D; ++c) {
        if (!bits[c] || !scale[c]) return fail(FA_ERR_ARG, "rot1 sum: client %d's %s is null", c, !bits[c] ? "bits" : "scale");
        if (!aligned(bits[c], 4) || !aligned(scale[c], 4))
            return fail(FA_ERR_ALIGN, "rot1 sum: client %d's %s not 4-byte aligned", c, !aligned(bits[c], 4) ? "bits" : "scale");
    }
    return FA_OK;
}

}  // namespace

extern "C" {

int fa_rot1_sum_host(const uint32_t* const* bits, const float* const* scale, const uint64_t* seed, const float* w, int D,
                     uint64_t idx0, size_t cnt, const float* ref, float* out) {
    g_err.clear();
    if (int rc = check_rot1_sum(reinterpret_cast<const void* const*>(bits), reinterpret_cast<const void* const*>(scale), seed, w,
                                D, cnt, idx0))
        return rc;
    if (cnt == 0) return FA_OK;
    if (!out) return fail(FA_ERR_ARG, "rot1 sum: out is null");
    fa::rot1_sum_host(bits, scale, seed, w, D, idx0, cnt, ref, out);
    return FA_OK;
}

int fa_rot1_sum_device(fa_ctx* ctx, int gpu, const uint32_t* const* d_bits, const float* const* d_scale, const uint64_t* seed,
                       const float* w, int D, uint64_t idx0, size_t cnt, const void* d_ref, fa_dtype ref_dtype, void* d_out,
                       fa_dtype out_dtype, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with cnt == 0 this is the feature probe of a box without a GPU
    if (!dvalid(out_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    FA_PAIR(ref_dtype, out_dtype);
    if (int rc = check_rot1_sum(reinterpret_cast<const void* const*>(d_bits), reinterpret_cast<const void* const*>(d_scale), seed,
                                w, D, cnt, idx0))
        return rc;
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (cnt == 0) return FA_OK;
    if (!d_out) return fail(FA_ERR_ARG, "rot1 sum: d_out is null");
    if (d_ref && !aligned(d_ref, dsize(ref_dtype)))
        return fail(FA_ERR_ALIGN, "rot1 sum: reference not %zu-byte aligned", dsize(ref_dtype));
    if (!aligned(d_out, dsize(out_dtype))) return fail(FA_ERR_ALIGN, "rot1 sum: output not %zu-byte aligned", dsize(out_dtype));
    if (d_ref) {
        const uintptr_t o = (uintptr_t)d_out, r = (uintptr_t)d_ref;
        if (o < r + cnt * dsize(ref_dtype) && r < o + cnt * dsize(out_dtype))
            return fail(FA_ERR_ARG, "rot1 sum: d_out overlaps d_ref");
    }
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_rot1_sum(d_bits, d_scale, seed, w, D, idx0, (int64_t)cnt, d_ref, ref_dtype, d_out, out_dtype, c.tu, c.s));
    return FA_OK;
}

}  // extern "C"
