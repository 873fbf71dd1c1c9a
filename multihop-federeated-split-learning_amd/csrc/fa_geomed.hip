// fa_geomed.hip -- the geomed stage's fused Weiszfeld pass (fa.h "Geomed stage", rule 1) for CDNA4 (gfx950): per
// element i the FA_FEDAVG chain v_i = fmaf(w_k, x_{k,i}, acc) over the nc clients of the pass, and for every
// client k, Q_k = sum_i ((double)fl32(x_{k,i} - v_i))^2 and B_k = the count of its elements that are NaN or +-inf.
//
// v_i depends only on the nc values of element i, and so does every difference against it: one kernel does both.
// A lane loads its bytes of every client first (all loads in flight before the first FMA), keeps them packed in
// registers, widens them once for the chain and once more for the differences against the chain's result.  The
// buckets are read from HBM once and v is never stored (unless the caller asks for it: the raw device entry and
// the tests).  The kernels are templated on the padded client count P = 2 .. 128 and fully unrolled, every index
// a compile-time constant, as in fa_trimmed.hip; clients nc .. P-1 are never read (client_live of fa_sortnet.h).
//
// Forms.  The vector form gives a lane 128 VGPRs of raw data whatever P is: 16-byte loads per client for P <= 32
// (the form of 32 clients), 8-byte loads for P = 64, 4-byte loads for P = 128 (the wide forms).  A 16-byte vector
// of the Split (fa_split.h) is 1, 2 or 4 such units, so the three widths share one split.  The element form, one
// element per lane, takes the head, the tail and inputs of mixed 16-byte phase for every P.
//
// Sums.  For P <= 32 a lane keeps one fp64 sum per client across all its tiles (2 P VGPRs) and the wave butterfly
// (wave_sum) runs once, at the end; for P = 64 and 128 there are no registers for that and the butterfly runs per
// tile.  Either way the wave's sum lands in one LDS cell per (wave, client), the four waves are added in wave order
// into one partial per (client, workgroup), and launch_measure_finish adds a client's partials in a fixed order:
// the clip kernel's reduction (fa_device.h, fa_clip.hip).  No atomics: one layout gives the same bits on every run.
// Non-finite inputs are rare, so the count costs the common tile one integer max per element and one ballot per
// client; only a wave that saw one counts, by ballots (exact integers), and lane 0 adds the count to the client's
// second LDS cell as an fp64 (exact below 2^53).  It travels through the same partials as row nc + k.
//
// Build: the client loops must unroll fully (the per-client registers are arrays indexed by the loop variable);
// `#pragma unroll` gives up above a cost limit that P = 128 exceeds, so the Makefile raises it for this TU.
//
// Numerics: the chain is __builtin_fmaf from +0 in client order, the bits of launch_chain; sq_add (fa_device.h) is
// the clip stage's d and q.  Contraction is off for the TU, as in fa_clip.hip.  A lane past the end of the data
// loads nothing and holds zeros; its v is forced to +0 (0 * an infinite weight would be NaN), so it adds +0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"
#include "fa_sortnet.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kGeoThreads = kMeasureThreads;
constexpr int kGeoLaneAccMaxP = 32;  // up to here a lane keeps its fp64 sums across tiles

// LDS rows: Q_k in row k, B_k in row nc + k.
using GeoLds = MeasureLds<2 * kMaxClients>;

// LW bytes of a bucket, non-temporal, in the low words of a u32x4 (the rest constant zeros: they cost no register).
template <int LW>
__device__ __forceinline__ u32x4 ld_raw(const void* p) {
    if constexpr (LW == 16) {
        return ld16<true>(p);
    } else if constexpr (LW == 8) {
        const u32x2 r = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
        return u32x4{r.x, r.y, 0u, 0u};
    } else {
        const uint32_t r = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
        return u32x4{r, 0u, 0u, 0u};
    }
}

// The first NW words of r made opaque to the compiler, at no instruction: between the two widenings of a 16-bit
// input, which it would otherwise merge into one, keeping every client's floats (twice the registers of the
// packed words) live across the chain.
template <int NW>
__device__ __forceinline__ void keep_packed(u32x4& r) {
    uint32_t a = r.x, b = r.y, c = r.z, d = r.w;
    asm("" : "+v"(a));
    if constexpr (NW >= 2) asm("" : "+v"(b));
    if constexpr (NW >= 4) {
        asm("" : "+v"(c));
        asm("" : "+v"(d));
    }
    r = u32x4{a, b, c, d};
}

// The kernel's client table -- its first argument, so the start of the kernel-argument segment -- through a pointer
// the compiler cannot see through, taken anew in every tile: the scalar loads of pointers and weights then sit
// where they are used.  Hoisted out of the tile loop, the 128 pointers and weights of the wide forms do not fit the
// SGPR file and went to scratch memory.
typedef const ClientTable __attribute__((address_space(4))) * TablePtr;
__device__ __forceinline__ TablePtr table_here() {
    uint64_t a = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return (TablePtr)a;
}

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
constexpr uint32_t kExpAllOnes = 0x7f800000u;  // |bits| at or above it: NaN or +-inf

// What one client's E differences of one lane add up to: a = the lane's fp64 sum so far, continued; the wave's
// count of non-finite inputs goes to LDS row brow at once (the rare path).
template <int E>
__device__ __forceinline__ double tally(const float* x, const float* v, double a, GeoLds& lds, int wave, int lane,
                                        int brow) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        a = sq_add(x[j], v[j], a);
        m = max(m, abs_bits(x[j]));
    }
    if (__ballot(m >= kExpAllOnes) != 0) {  // wave-uniform
        int c = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) c += __popcll(__ballot(abs_bits(x[j]) >= kExpAllOnes));
        if (lane == 0) lds.acc[wave][brow] += (double)c;
    }
    return a;
}

// Vector form: unit q of a bucket is its elements head + E q .. + E - 1, LW = E sizeof(T) bytes, LW-aligned in
// every client (head brings them to a 16-byte boundary).  Tile `tile` is units [256 tile, + 256), one per lane.
template <typename T, int P, int LW>
__global__ __launch_bounds__(kGeoThreads) void geomed_vec_kernel(const ClientTable t, int nc, float* v_out, int64_t head,
                                                                  int64_t nunits, double* partials, int64_t pstride) {
    constexpr int E = LW / (int)sizeof(T), V = In<T>::kVec;
    constexpr bool kLaneAcc = P <= kGeoLaneAccMaxP;
    __shared__ GeoLds lds;
    lds_zero(lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[kLaneAcc ? P : 1];
#pragma unroll
    for (int u = 0; u < (kLaneAcc ? P : 1); ++u) acc[u] = 0.0;
    const int64_t ntiles = (nunits + kGeoThreads - 1) / kGeoThreads;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t q = tile * kGeoThreads + threadIdx.x;
        const bool live = q < nunits;
        const int64_t e = head + (live ? q : 0) * E;
        const TablePtr tt = table_here();
        // every client's load in flight before the first FMA; two arrays of at most 64 clients: one of 128 was left
        // in scratch memory by the compiler
        u32x4 raw_lo[P < 64 ? P : 64], raw_hi[P > 64 ? P - 64 : 1];
#define FA_GEO_RAW(u) ((u) < 64 ? raw_lo[(u) < 64 ? (u) : 0] : raw_hi[(u) < 64 ? 0 : (u) - 64])
#pragma unroll
        for (int u = 0; u < P; ++u)
            if (client_live<P>(u, nc))
                FA_GEO_RAW(u) = live ? ld_raw<LW>(reinterpret_cast<const T*>(tt->src[u]) + e) : u32x4{};
        float v[E];
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] = 0.0f;
#pragma unroll
        for (int u = 0; u < P; ++u) {
            if (client_live<P>(u, nc)) {
                float x[V];
                In<T>::widen(FA_GEO_RAW(u), x);
                const float w = tt->w[u];
#pragma unroll
                for (int j = 0; j < E; ++j) v[j] = __builtin_fmaf(x[j], w, v[j]);
            }
        }
        if (!live) {
#pragma unroll
            for (int j = 0; j < E; ++j) v[j] = 0.0f;
        } else if (v_out) {
            float* o = v_out + e;  // (v_out + head) is 16-byte aligned: the Split requires it
            if constexpr (E >= 4) {
#pragma unroll
                for (int j = 0; j < E; j += 4) *reinterpret_cast<f32x4*>(o + j) = f32x4{v[j], v[j + 1], v[j + 2], v[j + 3]};
            } else {
#pragma unroll
                for (int j = 0; j < E; ++j) o[j] = v[j];
            }
        }
#pragma unroll
        for (int u = 0; u < P; ++u) {
            if (client_live<P>(u, nc)) {
                float x[V];
                if constexpr (sizeof(T) == 2) keep_packed<LW / 4>(FA_GEO_RAW(u));
                In<T>::widen(FA_GEO_RAW(u), x);
                if constexpr (kLaneAcc) {
                    acc[u] = tally<E>(x, v, acc[u], lds, wave, lane, nc + u);
                } else {
                    const double a = wave_sum(tally<E>(x, v, 0.0, lds, wave, lane, nc + u));
                    if (lane == 0) lds.acc[wave][u] += a;
                }
            }
        }
    }
    if constexpr (kLaneAcc) {
#pragma unroll
        for (int u = 0; u < P; ++u) {
            if (client_live<P>(u, nc)) {
                const double a = wave_sum(acc[u]);
                if (lane == 0) lds.acc[wave][u] += a;
            }
        }
    }
    lds_flush(lds, 2 * nc, partials, pstride, blockIdx.x);
}

#undef FA_GEO_RAW

// Element form over elements [0, head) and [tail0, n) (the whole array: head = tail0 = n), one element per lane
// and load; its partials go to slots slot0 + blockIdx.x.
template <typename T, int P>
__global__ __launch_bounds__(kGeoThreads) void geomed_elem_kernel(const ClientTable t, int nc, float* v_out, int64_t head,
                                                                   int64_t tail0, int64_t n, double* partials,
                                                                   int64_t pstride, int64_t slot0) {
    constexpr bool kLaneAcc = P <= kGeoLaneAccMaxP;
    __shared__ GeoLds lds;
    lds_zero(lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[kLaneAcc ? P : 1];
#pragma unroll
    for (int u = 0; u < (kLaneAcc ? P : 1); ++u) acc[u] = 0.0;
    const int64_t cnt = head + (n - tail0);
    const int64_t ntiles = (cnt + kGeoThreads - 1) / kGeoThreads;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t s = tile * kGeoThreads + threadIdx.x;
        const bool live = s < cnt;
        const int64_t i = !live ? 0 : s < head ? s : tail0 + (s - head);
        const TablePtr tt = table_here();
        float x_lo[P < 64 ? P : 64], x_hi[P > 64 ? P - 64 : 1];  // as the vector form's
#define FA_GEO_X(u) ((u) < 64 ? x_lo[(u) < 64 ? (u) : 0] : x_hi[(u) < 64 ? 0 : (u) - 64])
#pragma unroll
        for (int u = 0; u < P; ++u)
            if (client_live<P>(u, nc)) FA_GEO_X(u) = live ? In<T>::scalar(tt->src[u], i) : 0.0f;
        float v = 0.0f;
#pragma unroll
        for (int u = 0; u < P; ++u)
            if (client_live<P>(u, nc)) v = __builtin_fmaf(FA_GEO_X(u), tt->w[u], v);
        if (!live) v = 0.0f;
        else if (v_out) v_out[i] = v;
#pragma unroll
        for (int u = 0; u < P; ++u) {
            if (client_live<P>(u, nc)) {
                const float x = FA_GEO_X(u);
                if constexpr (kLaneAcc) {
                    acc[u] = tally<1>(&x, &v, acc[u], lds, wave, lane, nc + u);
                } else {
                    const double a = wave_sum(tally<1>(&x, &v, 0.0, lds, wave, lane, nc + u));
                    if (lane == 0) lds.acc[wave][u] += a;
                }
            }
        }
    }
    if constexpr (kLaneAcc) {
#pragma unroll
        for (int u = 0; u < P; ++u) {
            if (client_live<P>(u, nc)) {
                const double a = wave_sum(acc[u]);
                if (lane == 0) lds.acc[wave][u] += a;
            }
        }
    }
    lds_flush(lds, 2 * nc, partials, pstride, slot0 + blockIdx.x);
}

#undef FA_GEO_X

template <typename T, int P>
hipError_t launch_geomed_p(const ClientTable& t, int nc, float* v_out, const Split& sp, double* partials, double* sums,
                           const Tuning& tu, hipStream_t s) {
    constexpr int LW = P <= 32 ? 16 : P == 64 ? 8 : 4;  // 4 P VGPRs of raw data up to P = 32, 128 beyond
    constexpr int E = LW / (int)sizeof(T);
    const MeasureGrid gr = measure_grid(sp, (int64_t)kGeoThreads * E, kClipMaxBlocks, tu.max_blocks);
    const int64_t np = gr.np();
    if (gr.vec_blocks > 0) {
        hipLaunchKernelGGL((geomed_vec_kernel<T, P, LW>), dim3((unsigned)gr.vec_blocks), dim3(kGeoThreads), 0, s, t, nc,
                           v_out, sp.head, sp.nvec * (16 / LW), partials, np);
        if (gr.elem_blocks > 0)
            hipLaunchKernelGGL((geomed_elem_kernel<T, P>), dim3(1), dim3(kGeoThreads), 0, s, t, nc, v_out, sp.head,
                               sp.tail0(), sp.n, partials, np, gr.vec_blocks);
    } else {
        hipLaunchKernelGGL((geomed_elem_kernel<T, P>), dim3((unsigned)gr.elem_blocks), dim3(kGeoThreads), 0, s, t, nc,
                           v_out, sp.n, sp.n, sp.n, partials, np, (int64_t)0);
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return launch_measure_finish(partials, np, 2 * nc, sums, s);
}

template <typename T>
hipError_t launch_geomed_t(const ClientTable& t, int nc, float* v_out, const Split& sp, double* partials, double* sums,
                           const Tuning& tu, hipStream_t s) {
#define FA_GEO_P(P) \
    if (nc <= P) return launch_geomed_p<T, P>(t, nc, v_out, sp, partials, sums, tu, s)
    FA_GEO_P(2);
    FA_GEO_P(4);
    FA_GEO_P(8);
    FA_GEO_P(16);
    FA_GEO_P(32);
    FA_GEO_P(64);
#undef FA_GEO_P
    return launch_geomed_p<T, 128>(t, nc, v_out, sp, partials, sums, tu, s);
}

}  // namespace

hipError_t launch_geomed_pass(const ClientTable& t, int nc, fa_dtype in, float* v_out, const Split& sp, double* partials,
                              double* sums, const Tuning& tu, hipStream_t s) {
    if (!sp.valid() || sp.V != (in == FA_F32 ? 4 : 8)) return hipErrorInvalidValue;
    if (nc < 1 || nc > kMaxClients || sp.n <= 0 || !partials || !sums) return hipErrorInvalidValue;
    switch (in) {
        case FA_F32: return launch_geomed_t<float>(t, nc, v_out, sp, partials, sums, tu, s);
        case FA_BF16: return launch_geomed_t<uint16_t>(t, nc, v_out, sp, partials, sums, tu, s);
        case FA_F16: return launch_geomed_t<_Float16>(t, nc, v_out, sp, partials, sums, tu, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace fa
