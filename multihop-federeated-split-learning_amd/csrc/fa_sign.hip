// fa_sign.hip -- the sign-vote stage (fa.h "Sign-vote stage") for CDNA4 (gfx950): D one-bit receipts are counted per
// element without leaving the packed domain, the counts are compared against the vote's two thresholds bit-sliced, and
// only then is the fp32 side touched, once: a_i = fl32(widen(g_i) + t_i).  The kernel moves D / 8 + 8 bytes per element
// (f32) where the FMA chain over expanded slots moves 4 D + 4.
//
// Counting (count_planes).  A lane of the vector form loads 16 bytes -- four words, 128 elements -- of every receipt
// with nt loads, kGroup = 7 receipts in flight, and adds them as whole words: a full adder on three words is x = a ^ b,
// sum = x ^ c, carry = (x & c) | (~x & a) (one v_bfi_b32), three VALU instructions for 32 elements of three clients.
// Four full adders turn 7 words into a 3-bit number (12 instructions), a ripple adds it into the 8-plane counter (a half
// adder, two full adders, five half adders on the carry: 18), so a group costs 30 instructions per word, 4.3 per client
// and word, 0.13 per client and element.  No per-element integer exists.  A last group of fewer than 7 receipts takes
// zero words for the missing ones; the receipt pointers are read from the kernel arguments with scalar loads.
//
// Thresholds (ge_const, le_const).  neg_i is c_i >= ceil((D + m) / 2), pos_i is c_i <= floor((D - m) / 2).  Both
// constants are wave-uniform, so a comparator is a chain over the planes from the low bit up: c >= K takes r = p & r at
// a one bit of K and r = p | r at a zero bit, c <= K takes r = ~p | r and r = ~p & r.  Two mask words per 32 elements.
//
// Expansion, without LDS memory.  A wave's tile is 64 lanes x 128 = 8192 elements; lane l holds the masks of elements
// 128 l .. 128 l + 127 in four components of 32.  ds_bpermute_b32 reads one register of another lane, the same register
// for every reader, so the fp32 side walks the tile component by component: in step (c, t) lane j takes the vector
// V sub of component c of lane S t + j / P (f32: V = 4 elements per 16 bytes, P = 8 vectors per word, S = 8 source lanes
// per step, 8 steps per component; 16-bit references: V = 8, P = 4, S = 16, 4 steps), one permute per mask word, two per
// step; the mean rule permutes the 8 counter planes instead and rebuilds c_i from their bits.  Eight (four) neighbouring
// lanes then cover 128 contiguous bytes of g and of the output, the groups of a step lie 512 bytes apart, and the four
// components of a tile fill the gaps: a step's accesses are whole 128-byte lines, not one 1 KiB run.  (A walk with lane
// j on vector j + 64 r would need the component chosen by the reading lane, four permutes per mask.)  The four mask bits
// select -eta / +eta / +0 by v_cndmask, no branches; one 16-byte load of g, V single adds, one 16-byte store with
// policy sc1.  How the permutes and the strided lines behave in the memory pipeline is not measured.
//
// The element form (one word per lane, its 32 elements looped, the same adders on single words) runs the words before
// the first 16-byte boundary of the receipts, the words after the last whole 128 elements (the last partial word
// included), and the whole launch where the receipts disagree in their 16-byte phase or g, the output or the planes are
// not 16-byte aligned (sign_split).  The bits are the same either way: the counts are exact.
//
// Resources (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): the tile kernels of the majority rule
// take 111 - 112 VGPRs in every dtype pair (8 planes x 4 words, 7 x 4 words of receipts in flight, the masks and the
// hoisted loads of g), those of the mean rule 103 - 105; 0 AGPRs, no LDS, no scratch, no spills, 4 waves per SIMD.  The
// element kernels take 30 - 38 VGPRs, 8 waves per SIMD.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kGroup = 7;   // receipts per carry-save tree
constexpr int kPlanes = 8;  // counts 0 .. 128
constexpr int64_t kQuadElems = 128, kTileQuads = 64;
constexpr int64_t kMaxBlocks = 2048;  // 8 workgroups per CU on 256 CUs; tiles beyond it are strided
constexpr int64_t kElemMaxBlocks = 1 << 16;

struct SignTable {  // 1 KiB of the kernel-argument segment
    const uint32_t* bits[kMaxClients];
};

struct SignArgs {
    const void* ref;  // nullable: absolute mode
    void* out;
    uint32_t *neg, *pos;  // both or neither
    float eta;            // majority: eta; mean: step = fl32(eta / D)
    int D, tn, tp;        // the thresholds of neg and pos
    int64_t w0, nq;       // the vector form: its first word, its quads of 128 elements
    int64_t nwords, n;
};

template <class T>
__device__ __forceinline__ T splat(uint32_t v) {
    if constexpr (sizeof(T) == 4) return v;
    else return T{v, v, v, v};
}

template <class T>
__host__ __device__ __forceinline__ void full_add(T a, T b, T c, T& sum, T& carry) {
    const T x = a ^ b;
    sum = x ^ c;
    carry = (x & c) | (~x & a);
}

// p += x[0] + .. + x[6], bit-sliced.
template <class T>
__host__ __device__ __forceinline__ void add7(const T* x, T* p) {
    T s1, c1, s2, c2, b0, c3, b1, b2, k, t;
    full_add(x[0], x[1], x[2], s1, c1);
    full_add(x[3], x[4], x[5], s2, c2);
    full_add(s1, s2, x[6], b0, c3);
    full_add(c1, c2, c3, b1, b2);
    k = p[0] & b0;
    p[0] ^= b0;
    full_add(p[1], b1, k, t, k);
    p[1] = t;
    full_add(p[2], b2, k, t, k);
    p[2] = t;
#pragma unroll
    for (int b = 3; b < kPlanes; ++b) {
        t = p[b] & k;
        p[b] ^= k;
        k = t;
    }
}

// p := the counts of the D receipts' words load(bits) as 8 planes.
template <class T, class Load>
__device__ __forceinline__ void count_planes(const SignTable& tb, int D, Load load, T* p) {
#pragma unroll
    for (int b = 0; b < kPlanes; ++b) p[b] = splat<T>(0u);
    int k = 0;
    for (; k + kGroup <= D; k += kGroup) {
        T x[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) x[j] = load(tb.bits[k + j]);
        add7(x, p);
    }
    if (k < D) {  // wave-uniform
        T x[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            x[j] = splat<T>(0u);
            if (k + j < D) x[j] = load(tb.bits[k + j]);
        }
        add7(x, p);
    }
}

// c >= K and c <= K over the planes of c, 0 <= K < 2^kPlanes.
template <class T>
__device__ __forceinline__ T ge_const(const T* p, int K) {
    T r = splat<T>(~0u);
#pragma unroll
    for (int b = 0; b < kPlanes; ++b) r = (K >> b & 1) ? (p[b] & r) : (p[b] | r);
    return r;
}
template <class T>
__device__ __forceinline__ T le_const(const T* p, int K) {
    T r = splat<T>(~0u);
#pragma unroll
    for (int b = 0; b < kPlanes; ++b) r = (K >> b & 1) ? (~p[b] | r) : (~p[b] & r);
    return r;
}

__device__ __forceinline__ float vote_term(uint32_t neg, uint32_t pos, float eta) {
    const float up = (pos & 1u) ? eta : 0.0f;
    return (neg & 1u) ? -eta : up;
}
__device__ __forceinline__ float mean_term(const uint32_t* pw, int j, int D, float step) {
#pragma clang fp contract(off)
    uint32_t c = 0;
#pragma unroll
    for (int b = 0; b < kPlanes; ++b) c |= ((pw[b] >> j) & 1u) << b;
    const float s = (float)(D - 2 * (int)c);
    return s * step;
}
__device__ __forceinline__ float aggregate(bool rel, float g, float t) {
#pragma clang fp contract(off)
    const float sum = g + t;
    return rel ? sum : t;
}

__device__ __forceinline__ uint32_t lane_word(int src_lane, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}

// The vector form: a tile of 64 quads per wave and trip.  REF: the element type of g (of the output in absolute mode).
template <typename REF, typename OUT, int RULE>
__global__ __launch_bounds__(kThreads) void sign_tile_kernel(const SignTable tb, const SignArgs a) {
    constexpr int V = In<REF>::kVec, P = 32 / V, S = 64 / P, T = 64 / S;
    const int lane = (int)(threadIdx.x & 63u);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int from = lane / P, sh = V * (lane % P);
    const bool rel = a.ref != nullptr;
    const int64_t waves = (int64_t)gridDim.x * kWaves, ntile = (a.nq + kTileQuads - 1) / kTileQuads;
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + w; tile < ntile; tile += waves) {  // wave-uniform
        const int64_t q = tile * kTileQuads + lane;
        const bool mine = q < a.nq;  // a lane past the last quad counts the last one again and stores nothing
        const int64_t wq = a.w0 + 4 * (mine ? q : a.nq - 1);
        u32x4 p[kPlanes];
        count_planes<u32x4>(tb, a.D, [&](const uint32_t* b) { return ld16<true>(b + wq); }, p);
        u32x4 neg = u32x4{0, 0, 0, 0}, pos = u32x4{0, 0, 0, 0};
        if constexpr (RULE == FA_SIGN_MAJORITY) {
            neg = ge_const(p, a.tn);
            pos = le_const(p, a.tp);
            if (a.neg && mine) {
                *reinterpret_cast<u32x4*>(a.neg + wq) = neg;
                *reinterpret_cast<u32x4*>(a.pos + wq) = pos;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll 2
            for (int t = 0; t < T; ++t) {
                const int src = S * t + from;  // every lane permutes: the stores alone are predicated
                uint32_t pw[kPlanes], nw = 0, ow = 0;
                if constexpr (RULE == FA_SIGN_MAJORITY) {
                    nw = lane_word(src, neg[c]) >> sh;
                    ow = lane_word(src, pos[c]) >> sh;
                } else {
#pragma unroll
                    for (int b = 0; b < kPlanes; ++b) pw[b] = lane_word(src, p[b][c]) >> sh;
                }
                const int64_t sq = tile * kTileQuads + src;
                if (sq < a.nq) {
                    const int64_t e = 32 * a.w0 + kQuadElems * sq + 32 * c + sh;
                    float g[V], r[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) g[j] = 0.0f;
                    if (rel) In<REF>::widen(ld16<true>(static_cast<const REF*>(a.ref) + e), g);
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        float tj;
                        if constexpr (RULE == FA_SIGN_MAJORITY) tj = vote_term(nw >> j, ow >> j, a.eta);
                        else tj = mean_term(pw, j, a.D, a.eta);
                        r[j] = aggregate(rel, g[j], tj);
                    }
                    Out<OUT>::template store<V, kStSc1>(a.out, e, r);
                }
            }
        }
    }
}

// The element form over words [0, headw) and [tailw0, nwords) (the whole launch: headw = tailw0 = nwords), one word per
// lane and trip; elements at or beyond n are neither read nor written, their plane bits are 0.
template <typename REF, typename OUT, int RULE>
__global__ __launch_bounds__(kThreads) void sign_elem_kernel(const SignTable tb, const SignArgs a, int64_t headw,
                                                             int64_t tailw0) {
    const bool rel = a.ref != nullptr;
    const int64_t cnt = headw + (a.nwords - tailw0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cnt; s += stride) {
        const int64_t wi = s < headw ? s : tailw0 + (s - headw);
        uint32_t p[kPlanes];
        count_planes<uint32_t>(tb, a.D, [&](const uint32_t* b) { return __builtin_nontemporal_load(b + wi); }, p);
        const int64_t e0 = 32 * wi;
        const int live = (int)(a.n - e0 < 32 ? a.n - e0 : 32);
        const uint32_t mask = live == 32 ? ~0u : (1u << live) - 1u;
        uint32_t neg = 0, pos = 0;
        if constexpr (RULE == FA_SIGN_MAJORITY) {
            neg = ge_const(p, a.tn) & mask;
            pos = le_const(p, a.tp) & mask;
            if (a.neg) {
                a.neg[wi] = neg;
                a.pos[wi] = pos;
            }
        }
#pragma clang loop unroll(disable)
        for (int j = 0; j < live; ++j) {
            float tj;
            if constexpr (RULE == FA_SIGN_MAJORITY) tj = vote_term(neg >> j, pos >> j, a.eta);
            else tj = mean_term(p, j, a.D, a.eta);
            const float g = rel ? In<REF>::scalar(a.ref, e0 + j) : 0.0f;
            Out<OUT>::scalar(a.out, e0 + j, aggregate(rel, g, tj));
        }
    }
}

template <typename REF, typename OUT, int RULE>
hipError_t launch_sign_t(const SignTable& tb, SignArgs a, const SignSplit& sp, const Tuning& tu, hipStream_t s) {
    const int64_t cap = tu.max_blocks > 0 ? std::min<int64_t>(kMaxBlocks, tu.max_blocks) : kMaxBlocks;
    if (sp.vec && sp.nq > 0) {
        a.w0 = sp.headw;
        a.nq = sp.nq;
        const int64_t ntile = (sp.nq + kTileQuads - 1) / kTileQuads;
        hipLaunchKernelGGL((sign_tile_kernel<REF, OUT, RULE>), dim3((unsigned)std::min((ntile + kWaves - 1) / kWaves, cap)),
                           dim3(kThreads), 0, s, tb, a);
        if (sp.edge_words() > 0)
            hipLaunchKernelGGL((sign_elem_kernel<REF, OUT, RULE>), dim3(1), dim3(64), 0, s, tb, a, sp.headw, sp.tailw0());
        return hipGetLastError();
    }
    const int64_t blocks = std::max<int64_t>(1, std::min((sp.nwords + kThreads - 1) / kThreads, std::min(cap * 32, kElemMaxBlocks)));
    hipLaunchKernelGGL((sign_elem_kernel<REF, OUT, RULE>), dim3((unsigned)blocks), dim3(kThreads), 0, s, tb, a, sp.nwords,
                       sp.nwords);
    return hipGetLastError();
}

template <typename REF, typename OUT>
hipError_t launch_sign_r(int rule, const SignTable& tb, const SignArgs& a, const SignSplit& sp, const Tuning& tu, hipStream_t s) {
    return rule == FA_SIGN_MEAN ? launch_sign_t<REF, OUT, FA_SIGN_MEAN>(tb, a, sp, tu, s)
                                : launch_sign_t<REF, OUT, FA_SIGN_MAJORITY>(tb, a, sp, tu, s);
}

// The element type the kernels are built on: the reference's, or in absolute mode the output's.
inline fa_dtype lead_dtype(const void* ref, fa_dtype rdt, fa_dtype odt) { return ref ? rdt : odt; }

}  // namespace

SignSplit sign_split(const uint32_t* const* bits, int D, size_t n, const void* ref, fa_dtype rdt, const void* out,
                     fa_dtype odt, const void* neg, const void* pos) {
    SignSplit sp{0, 0, (int64_t)((n + 31) / 32), true};
    const uintptr_t phase = (uintptr_t)bits[0] % 16;
    for (int k = 0; k < D; ++k) sp.vec = sp.vec && (uintptr_t)bits[k] % 16 == phase && phase % 4 == 0;
    if (neg) sp.vec = sp.vec && (uintptr_t)neg % 16 == phase && (uintptr_t)pos % 16 == phase;
    const size_t V = lead_dtype(ref, rdt, odt) == FA_F32 ? 4 : 8, so = odt == FA_F32 ? 4 : 2;
    sp.vec = sp.vec && (uintptr_t)ref % 16 == 0 && (uintptr_t)out % std::min<size_t>(16, V * so) == 0;
    sp.headw = std::min<int64_t>((int64_t)((16 - phase) % 16 / 4), sp.nwords);
    sp.nq = sp.vec && (int64_t)n >= 32 * sp.headw ? ((int64_t)n - 32 * sp.headw) / kQuadElems : 0;
    if (sp.nq == 0) sp.vec = false;
    return sp;
}

hipError_t launch_sign_vote(const uint32_t* const* bits, int D, int64_t n, float eta, int rule, int margin, const void* ref,
                            fa_dtype rdt, void* out, fa_dtype odt, uint32_t* neg, uint32_t* pos, const SignSplit& sp,
                            const Tuning& tu, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (D < 1 || D > kMaxClients || margin < 1 || margin > D || !out || (neg == nullptr) != (pos == nullptr) ||
        (rule != FA_SIGN_MAJORITY && rule != FA_SIGN_MEAN) || (rule == FA_SIGN_MEAN && neg) ||
        sp.nwords != (n + 31) / 32 || (sp.vec && (sp.headw < 0 || sp.nq < 1 || 32 * sp.headw + kQuadElems * sp.nq > n)))
        return hipErrorInvalidValue;
    SignTable tb;
    for (int k = 0; k < D; ++k) tb.bits[k] = bits[k];
    for (int k = D; k < kMaxClients; ++k) tb.bits[k] = nullptr;
    SignArgs a{ref, out, neg, pos, rule == FA_SIGN_MEAN ? eta / (float)D : eta, D, (D + margin + 1) / 2, (D - margin) / 2,
               0, 0, sp.nwords, n};
    const fa_dtype lead = lead_dtype(ref, rdt, odt);
    if (!dtype_pair_ok(lead, odt)) return hipErrorInvalidValue;
    switch (lead) {
        case FA_F32:
            return odt == FA_F32    ? launch_sign_r<float, float>(rule, tb, a, sp, tu, s)
                   : odt == FA_BF16 ? launch_sign_r<float, uint16_t>(rule, tb, a, sp, tu, s)
                                    : launch_sign_r<float, _Float16>(rule, tb, a, sp, tu, s);
        case FA_BF16:
            return odt == FA_F32 ? launch_sign_r<uint16_t, float>(rule, tb, a, sp, tu, s)
                                 : launch_sign_r<uint16_t, uint16_t>(rule, tb, a, sp, tu, s);
        case FA_F16:
            return odt == FA_F32 ? launch_sign_r<_Float16, float>(rule, tb, a, sp, tu, s)
                                 : launch_sign_r<_Float16, _Float16>(rule, tb, a, sp, tu, s);
    }
    return hipErrorInvalidValue;
}

void sign_pack_host(const float* delta, size_t n, uint32_t* bits) {
    for (size_t w = 0; w < (n + 31) / 32; ++w) bits[w] = 0u;
    for (size_t i = 0; i < n; ++i)
        if (delta[i] < 0.0f) bits[i >> 5] |= 1u << (i & 31);
}

void sign_vote_host(const uint32_t* const* bits, int D, size_t n, uint64_t idx0, float eta, int rule, int margin,
                    const float* ref, float* out, uint32_t* neg, uint32_t* pos) {
#pragma clang fp contract(off)
    const float step = eta / (float)D;
    for (size_t w = 0; neg && w < (n + 31) / 32; ++w) neg[w] = pos[w] = 0u;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t e = idx0 + i;
        int c = 0;
        for (int k = 0; k < D; ++k) c += (int)(bits[k][e >> 5] >> (e & 31) & 1u);
        const int sgn = D - 2 * c;
        float t;
        if (rule == FA_SIGN_MEAN) {
            t = (float)sgn * step;
        } else {
            const int v = sgn >= margin ? 1 : -sgn >= margin ? -1 : 0;
            t = v > 0 ? eta : v < 0 ? -eta : 0.0f;
            if (neg && v < 0) neg[i >> 5] |= 1u << (i & 31);
            if (neg && v > 0) pos[i >> 5] |= 1u << (i & 31);
        }
        out[i] = ref ? ref[i] + t : t;
    }
}

}  // namespace fa
