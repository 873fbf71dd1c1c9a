// fa_krum.hip -- the Krum stage's distance pass (fa.h "Krum stage", rule 1) for CDNA4 (gfx950): for every
// unordered pair a < b of the D clients of a pass, Q_ab = sum_i ((double)fl32(x_{a,i} - x_{b,i}))^2 over the n
// elements of a bucket.  O(D^2 n) arithmetic over O(D n) bytes: every bucket is read from HBM once.
//
// A workgroup of 256 lanes owns tiles of E elements of all D clients (E a power of two, E D about 8192).  It
// stages a tile in LDS as [client][element] fp32, rows E + 4 floats apart (the loads of one wave are 1 KiB
// runs of one client; the 4 floats of padding put consecutive clients 4 banks apart), dead elements and dead
// clients as zeros.  The pairs are cut into 4 x 4 blocks: with B = ceil(D / 4), block (bi, bj), bi <= bj,
// holds the pairs of clients {bi, bi + B, bi + 2B, bi + 3B} with {bj, bj + B, bj + 2B, bj + 3B} -- every
// unordered pair lies in exactly one block (the blocks bi == bj keep their pairs above the diagonal, clients
// >= D are dead).  A lane owns a block and keeps its 16 fp64 sums in registers: per group of 4 elements it
// reads its 8 clients with 8 ds_read_b128 (lanes of consecutive bj read consecutive 16-byte slots, lanes of
// one bi the same address) for 64 fused multiply-adds.  With NB = B (B + 1) / 2 <= 256 blocks the workgroup
// runs S = 256 / NB slices of lanes, slice s taking the element groups s, s + S, ...; with more blocks (D > 88)
// a lane owns up to 3 of them.  At the end the slices' sums are added in slice order through LDS and every
// live pair's sum goes to its slot partials[pair][workgroup].  A second launch, one wave per pair, adds a
// pair's partials (lane l takes l, l + 64, ... in ascending order, then an xor butterfly) and writes both
// mirror entries of the D x D matrix, whose diagonal is +0 without being computed.  No atomic anywhere, so
// for one layout (n, D, grid, pointer phases) every run gives the same bits; the order itself is not part of
// the rule (fa.h bounds the error of any order).
//
// Numerics: sq_add of fa_device.h, shared with fa_clip.hip (one fp32 subtraction of the exactly widened inputs,
// an exact fp64 square, the single rounding of the add).  Contraction is off for the TU.  The grid is
// measure_grid of fa_split.h over tiles of E elements.
//
// Two forms, as the other kernel TUs: the vector form fills the tile with 16-byte non-temporal loads when
// every client shares one 16-byte phase; the element form (one element per lane and load) fills it for the
// head, the tail and mixed phases.  Both run the same accumulation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kKrumThreads = 256;
constexpr int kKrumLdsFloats = 8704;  // 34 KiB: 128 clients x (64 + 4), and 256 lanes x 16 fp64 sums
constexpr int kKrumRowPad = 4;

// The geometry of a pass over D clients (host-computed, the same in every workgroup).
struct KrumGeom {
    int D, B, NB;  // clients, rows of 4 x 4 blocks, blocks
    int E, RS;     // elements per tile, floats between two clients' rows
    int S;         // slices of lanes (1 when a lane owns several blocks)
};

KrumGeom krum_geom(int D) {
    KrumGeom g;
    g.D = D;
    g.B = (D + 3) / 4;
    g.NB = g.B * (g.B + 1) / 2;
    g.E = 2048;
    while (4 * g.B * (g.E + kKrumRowPad) > kKrumLdsFloats) g.E >>= 1;  // >= 64 at B = 32
    g.RS = g.E + kKrumRowPad;
    g.S = g.NB > kKrumThreads ? 1 : std::min(kKrumThreads / g.NB, g.E / 4);
    return g;
}

__host__ __device__ inline int64_t pair_index(int lo, int hi, int D) {
    return (int64_t)lo * (2 * D - lo - 1) / 2 + (hi - lo - 1);
}

// Block blk of the row-major upper triangle of B x B blocks.
__device__ __forceinline__ void block_of(int blk, int B, int* bi, int* bj) {
    int i = 0, r = blk;
    while (r >= B - i) {
        r -= B - i;
        ++i;
    }
    *bi = i;
    *bj = i + r;
}

// What a lane owns: NBL blocks (on[q]: it has a q-th one) and a slice of the element groups.
template <int NBL>
struct KrumLane {
    int bi[NBL], bj[NBL];
    bool on[NBL];
    int g0, gstep;  // element groups g0, g0 + gstep, ...
    double acc[NBL][16];
};

template <int NBL>
__device__ __forceinline__ void lane_init(KrumLane<NBL>& L, const KrumGeom& gm) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NBL; ++q) {
        int blk;
        if (gm.S > 1 || NBL == 1) {
            blk = t % gm.NB;
            L.on[q] = q == 0 && t < gm.S * gm.NB;
        } else {
            blk = t + q * kKrumThreads;
            L.on[q] = blk < gm.NB;
        }
        L.bi[q] = L.bj[q] = 0;
        if (L.on[q]) block_of(blk, gm.B, &L.bi[q], &L.bj[q]);
#pragma unroll
        for (int p = 0; p < 16; ++p) L.acc[q][p] = 0.0;
    }
    L.g0 = gm.S > 1 ? t / gm.NB : 0;
    L.gstep = gm.S;
}

// The tile's first `groups` groups of 4 elements into the lane's sums.
template <int NBL>
__device__ __forceinline__ void accumulate(KrumLane<NBL>& L, const float* tile, const KrumGeom& gm, int groups) {
    for (int g = L.g0; g < groups; g += L.gstep) {
#pragma unroll
        for (int q = 0; q < NBL; ++q) {
            if (!L.on[q]) continue;
            f32x4 xa[4], xb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                xa[a] = *reinterpret_cast<const f32x4*>(tile + (L.bi[q] + a * gm.B) * gm.RS + 4 * g);
                xb[a] = *reinterpret_cast<const f32x4*>(tile + (L.bj[q] + a * gm.B) * gm.RS + 4 * g);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int j = 0; j < 4; ++j) L.acc[q][a * 4 + b] = sq_add(xa[a][j], xb[b][j], L.acc[q][a * 4 + b]);
        }
    }
}

// The sum of entry p (a = p / 4, b = p % 4) of block (bi, bj) into the workgroup's slot of its pair, if the
// pair is live.
__device__ __forceinline__ void store_pair(const KrumGeom& gm, int bi, int bj, int p, double v, double* partials,
                                           int64_t pstride, int64_t slot) {
    const int a = p >> 2, b = p & 3;
    const int ka = bi + a * gm.B, kb = bj + b * gm.B;
    if (ka >= gm.D || kb >= gm.D || ka == kb || (bi == bj && a >= b)) return;
    partials[pair_index(ka < kb ? ka : kb, ka < kb ? kb : ka, gm.D) * pstride + slot] = v;
}

// After the last tile: the slices' sums added in slice order (through the LDS the tiles used), then stored.
template <int NBL>
__device__ __forceinline__ void flush(KrumLane<NBL>& L, float* tile, const KrumGeom& gm, double* partials,
                                      int64_t pstride, int64_t slot) {
    if (gm.S == 1) {
#pragma unroll
        for (int q = 0; q < NBL; ++q)
            if (L.on[q])
#pragma unroll
                for (int p = 0; p < 16; ++p) store_pair(gm, L.bi[q], L.bj[q], p, L.acc[q][p], partials, pstride, slot);
        return;
    }
    double* red = reinterpret_cast<double*>(tile);  // S * NB * 16 <= 256 * 16 doubles
    __syncthreads();
    if (L.on[0]) {
        const int blk = threadIdx.x % gm.NB;
#pragma unroll
        for (int p = 0; p < 16; ++p) red[((int64_t)L.g0 * gm.NB + blk) * 16 + p] = L.acc[0][p];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < gm.NB * 16; o += kKrumThreads) {
        double v = red[o];
        for (int s = 1; s < gm.S; ++s) v += red[(int64_t)s * gm.NB * 16 + o];
        int bi, bj;
        block_of(o >> 4, gm.B, &bi, &bj);
        store_pair(gm, bi, bj, o & 15, v, partials, pstride, slot);
    }
}

// The clients' pointers in LDS (a lane picks its client by a per-lane index, which the kernel-argument
// table cannot serve), and zeros in the whole tile: the rows of dead clients stay zero.
__device__ __forceinline__ void stage_init(const ClientTable& t, const KrumGeom& gm, const void** ptrs, float* tile) {
    for (int k = 0; k < gm.D; ++k)  // k is uniform: scalar loads from the kernel arguments
        if (threadIdx.x == 0) ptrs[k] = t.src[k];
    for (int i = threadIdx.x; i < kKrumLdsFloats; i += kKrumThreads) tile[i] = 0.0f;
    __syncthreads();
}

// Vector form: vector v of a bucket is elements head + V v .. + V - 1, 16-byte aligned in every client.  Tile
// `tile` is vectors [tile * E / V, + E / V) of every client.
template <typename T, int NBL>
__global__ __launch_bounds__(kKrumThreads) void pairdist_vec_kernel(const ClientTable t, const KrumGeom gm,
                                                                     int64_t head, int64_t nvec, double* partials,
                                                                     int64_t pstride) {
    constexpr int V = In<T>::kVec, U = 4;
    __shared__ __attribute__((aligned(16))) float tile[kKrumLdsFloats];
    __shared__ const void* ptrs[kMaxClients];
    stage_init(t, gm, ptrs, tile);
    KrumLane<NBL> L;
    lane_init(L, gm);
    const int EV = gm.E / V;  // vectors of one client in a tile, a power of two
    const int total = gm.D * EV;
    const int64_t ntiles = (nvec + EV - 1) / EV;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int64_t v0 = tl * EV;
        const int live = nvec - v0 < EV ? (int)(nvec - v0) : EV;  // vectors of a client in this tile
        for (int i0 = threadIdx.x; i0 < total; i0 += U * kKrumThreads) {
            u32x4 r[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * kKrumThreads;
                const int k = i / EV, v = i % EV;
                r[u] = u32x4{};
                if (i < total && v < live) r[u] = ld16<true>(reinterpret_cast<const T*>(ptrs[k]) + head + (v0 + v) * V);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * kKrumThreads;
                if (i >= total) continue;
                const int k = i / EV, v = i % EV;
                float x[V];
                In<T>::widen(r[u], x);
                float* dst = tile + k * gm.RS + v * V;
#pragma unroll
                for (int j = 0; j < V; j += 4) *reinterpret_cast<f32x4*>(dst + j) = f32x4{x[j], x[j + 1], x[j + 2], x[j + 3]};
            }
        }
        __syncthreads();
        accumulate(L, tile, gm, (live * V + 3) / 4);
        __syncthreads();
    }
    flush(L, tile, gm, partials, pstride, blockIdx.x);
}

// Element form over elements [0, head) and [tail0, n) (the whole array: head = tail0 = n), one element per lane
// and load; its partials go to slots slot0 + blockIdx.x.
template <typename T, int NBL>
__global__ __launch_bounds__(kKrumThreads) void pairdist_elem_kernel(const ClientTable t, const KrumGeom gm,
                                                                      int64_t head, int64_t tail0, int64_t n,
                                                                      double* partials, int64_t pstride, int64_t slot0) {
    __shared__ __attribute__((aligned(16))) float tile[kKrumLdsFloats];
    __shared__ const void* ptrs[kMaxClients];
    stage_init(t, gm, ptrs, tile);
    KrumLane<NBL> L;
    lane_init(L, gm);
    const int64_t cnt = head + (n - tail0);
    const int total = gm.D * gm.E;
    const int64_t ntiles = (cnt + gm.E - 1) / gm.E;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int64_t s0 = tl * gm.E;
        const int live = cnt - s0 < gm.E ? (int)(cnt - s0) : gm.E;
        const int fill = (live + 3) / 4 * 4;  // what accumulate reads of a row
        for (int i = threadIdx.x; i < total; i += kKrumThreads) {
            const int k = i / gm.E, e = i % gm.E;
            if (e >= fill) continue;
            float x = 0.0f;
            if (e < live) {
                const int64_t s = s0 + e;
                x = In<T>::scalar(ptrs[k], s < head ? s : tail0 + (s - head));
            }
            tile[k * gm.RS + e] = x;
        }
        __syncthreads();
        accumulate(L, tile, gm, (live + 3) / 4);
        __syncthreads();
    }
    flush(L, tile, gm, partials, pstride, slot0 + blockIdx.x);
}

// One wave per pair: dist[a][b] = dist[b][a] = the pair's np partials, lane l adding l, l + 64, ... in
// ascending order.
__global__ __launch_bounds__(64) void pairdist_finish_kernel(const double* partials, int64_t pstride, int64_t np, int D,
                                                             double* dist) {
    int a = 0, r = blockIdx.x;
    while (r >= D - 1 - a) {
        r -= D - 1 - a;
        ++a;
    }
    const int b = a + 1 + r;
    const double* p = partials + (int64_t)blockIdx.x * pstride;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < np; i += 64) v += p[i];
    v = wave_sum(v);
    if (threadIdx.x == 0) {
        dist[(int64_t)a * D + b] = v;
        dist[(int64_t)b * D + a] = v;
    }
}

template <typename T, int NBL>
hipError_t launch_pairdist_t(const ClientTable& t, const KrumGeom& gm, const Split& sp, double* partials, double* dist,
                             const Tuning& tu, hipStream_t s) {
    const MeasureGrid gr = measure_grid(sp, gm.E, kKrumMaxBlocks, tu.max_blocks);
    const int64_t vec_blocks = gr.vec_blocks, elem_blocks = gr.elem_blocks, np = gr.np();
    if (vec_blocks > 0) {
        hipLaunchKernelGGL((pairdist_vec_kernel<T, NBL>), dim3((unsigned)vec_blocks), dim3(kKrumThreads), 0, s, t, gm,
                           sp.head, sp.nvec, partials, np);
        if (elem_blocks > 0)
            hipLaunchKernelGGL((pairdist_elem_kernel<T, NBL>), dim3(1), dim3(kKrumThreads), 0, s, t, gm, sp.head,
                               sp.tail0(), sp.n, partials, np, vec_blocks);
    } else {
        hipLaunchKernelGGL((pairdist_elem_kernel<T, NBL>), dim3((unsigned)elem_blocks), dim3(kKrumThreads), 0, s, t, gm,
                           sp.n, sp.n, sp.n, partials, np, (int64_t)0);
    }
    hipLaunchKernelGGL(pairdist_finish_kernel, dim3((unsigned)krum_pairs(gm.D)), dim3(64), 0, s, partials, np, np, gm.D,
                       dist);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_pairdist_nbl(const ClientTable& t, const KrumGeom& gm, const Split& sp, double* partials,
                               double* dist, const Tuning& tu, hipStream_t s) {
    if (gm.NB <= kKrumThreads) return launch_pairdist_t<T, 1>(t, gm, sp, partials, dist, tu, s);
    if (gm.NB <= 2 * kKrumThreads) return launch_pairdist_t<T, 2>(t, gm, sp, partials, dist, tu, s);
    return launch_pairdist_t<T, 3>(t, gm, sp, partials, dist, tu, s);  // NB <= 528 at D = 128
}

}  // namespace

hipError_t launch_pairdist(const ClientTable& t, int D, fa_dtype in, const Split& sp, double* partials, double* dist,
                           const Tuning& tu, hipStream_t s) {
    if (!sp.valid() || sp.V != (in == FA_F32 ? 4 : 8)) return hipErrorInvalidValue;
    if (D < 1 || D > kMaxClients || sp.n <= 0 || !dist || (D > 1 && !partials)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(dist, 0, (size_t)D * D * sizeof(double), s);  // the diagonal is +0
    if (e != hipSuccess || D == 1) return e;
    const KrumGeom gm = krum_geom(D);
    switch (in) {
        case FA_F32: return launch_pairdist_nbl<float>(t, gm, sp, partials, dist, tu, s);
        case FA_BF16: return launch_pairdist_nbl<uint16_t>(t, gm, sp, partials, dist, tu, s);
        case FA_F16: return launch_pairdist_nbl<_Float16>(t, gm, sp, partials, dist, tu, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace fa
