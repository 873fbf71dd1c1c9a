// fa_gram.hip -- the Gram pass (fa.h "Gram pass") for CDNA4 (gfx950): G_ab = sum_i (double)y_a,i (double)y_b,i over
// the n elements of the D <= 128 clients of a pass, y the exactly widened input or fl32(widen(x) - ref_i).  O(D^2 n)
// multiply-adds over O(D n) bytes, every bucket read from HBM once, and the D^2 part on the matrix unit:
// v_mfma_f64_16x16x4_f64 multiplies a 16 x 4 by a 4 x 16 block of doubles, 1024 exact products per issue.
//
// The clients are padded to B = ceil(D / 16) blocks of 16.  A workgroup of 256 lanes (4 waves) owns tiles of E
// elements of all clients (E = 256, 128, 64, 64, 32 .. 32 for B = 1 .. 8) and stages a tile in LDS as [client][element]
// of values already converted to fp64, one conversion (and one fp32 subtract under a reference) per element; rows
// are E + 2 doubles apart, dead elements and dead clients are zeros.  For the MFMA the operand of lane l for client
// block b at k-step s is the one double Y[16 b + l % 16][4 s + l / 16], and it is the A operand of every block pair
// (b, .) and the B operand of every pair (., b): per k-step a wave reads B <= 8 doubles (one ds_read_b64 each) and
// issues one MFMA per block pair it owns.  The NP = B (B + 1) / 2 <= 36 block pairs bi <= bj (row-major upper
// triangle) are dealt over the waves, pair p to wave p % 4, at most 9 pairs = 36 accumulator doubles per lane; with
// NP < 4 (D <= 32) every wave owns all pairs and takes the k-steps w, w + 4, ... of a tile instead, and the waves'
// sums are added through LDS in wave order after the last tile.  Row padding: within the lanes 0 .. 31 of a read
// (l % 16 = r, l / 16 = c in {0, 1}) the doubles lie (E + 2) r + c apart, which is 2 r + c modulo 32 as E is a
// multiple of 32: 32 different 8-byte columns of the 64 four-byte banks, and the same for lanes 32 .. 63.
//
// The accumulators stay in registers across the grid-stride loop over tiles; the vector form holds the next tile's
// 16-byte global loads in registers while the MFMAs of this one run.  At the end each workgroup writes one partial
// per (entry a <= b, workgroup) -- register r of lane l of pair (bi, bj) is G[16 bi + 4 r + l / 16][16 bj + l % 16] --
// and a second launch, one wave per entry, adds an entry's partials (lane l takes l, l + 64, ... in ascending order,
// then an xor butterfly) and writes both mirror entries.  No atomic anywhere: for one layout every run gives the same
// bits; the order itself is not part of the rule.  Contraction is off for the TU.
//
// Two forms, as the other kernel TUs, which differ only in the fill: 16-byte non-temporal loads when every client
// (and the reference) shares one 16-byte phase; one element per lane and load for the head, the tail and mixed phases.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "fa_device.h"
#include "fa_internal.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kGramThreads = 256, kGramWaves = kGramThreads / 64;
constexpr int kGramRowPad = 2;
constexpr int kGramLdsDoubles = 128 * (32 + kGramRowPad);  // 34 KiB: 128 clients x (32 + 2), 16 x (256 + 2) fits too

// Block pair p of the row-major upper triangle of B x B blocks.
__host__ __device__ constexpr int pair_bi(int B, int p) {
    int i = 0;
    while (p >= B - i) {
        p -= B - i;
        ++i;
    }
    return i;
}
__host__ __device__ constexpr int pair_bj(int B, int p) {
    int i = 0;
    while (p >= B - i) {
        p -= B - i;
        ++i;
    }
    return i + p;
}

// The geometry of a pass over B blocks of 16 clients.
template <int B>
struct GramGeom {
    static constexpr int NP = B * (B + 1) / 2;      // block pairs
    static constexpr bool kSplit = NP < kGramWaves;  // the waves split the k-steps, not the pairs
    static constexpr int NPW = kSplit ? NP : (NP + kGramWaves - 1) / kGramWaves;  // accumulators of a wave
    static constexpr int E = gram_tile(B), RS = E + kGramRowPad;
    static_assert(E % 32 == 0 && 16 * B * RS <= kGramLdsDoubles, "the tile fits and rows are 2 modulo 32 apart");
    static_assert(!kSplit || kGramWaves * NP * 256 <= kGramLdsDoubles, "the waves' sums fit the tile's LDS");
};

// Entry (a, b), a <= b, of the row-major upper triangle with its diagonal.
__device__ __forceinline__ int64_t gram_index(int a, int b, int D) { return (int64_t)a * (2 * D - a + 1) / 2 + (b - a); }

template <int B, int P>
__device__ __forceinline__ void mma_pair(const double (&a)[B], f64x4 (&acc)[GramGeom<B>::NPW], int wave) {
    constexpr int bi = pair_bi(B, P), bj = pair_bj(B, P);
    if constexpr (GramGeom<B>::kSplit) {
        acc[P] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], a[bj], acc[P], 0, 0, 0);
    } else {
        if ((P % kGramWaves) == wave)  // uniform in a wave
            acc[P / kGramWaves] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], a[bj], acc[P / kGramWaves], 0, 0, 0);
    }
}
template <int B, int... P>
__device__ __forceinline__ void mma_pairs(std::integer_sequence<int, P...>, const double (&a)[B],
                                          f64x4 (&acc)[GramGeom<B>::NPW], int wave) {
    (mma_pair<B, P>(a, acc, wave), ...);
}

// The tile's first `steps` k-steps of 4 elements into the wave's sums.
template <int B>
__device__ __forceinline__ void accumulate(f64x4 (&acc)[GramGeom<B>::NPW], const double* tile, int steps, int wave, int lane) {
    using G = GramGeom<B>;
    const double* base = tile + (lane & 15) * G::RS + (lane >> 4);
    for (int s = G::kSplit ? wave : 0; s < steps; s += G::kSplit ? kGramWaves : 1) {
        double a[B];
#pragma unroll
        for (int b = 0; b < B; ++b) a[b] = base[b * 16 * G::RS + 4 * s];
        mma_pairs<B>(std::make_integer_sequence<int, G::NP>{}, a, acc, wave);
    }
}

// Register r of `lane` of block pair p: the workgroup's sum of one entry into its slot, if the entry is live and on
// or above the diagonal.
template <int B>
__device__ __forceinline__ void store_entry(int D, int p, int r, int lane, double v, double* partials, int64_t pstride,
                                            int64_t slot) {
    const int bi = pair_bi(B, p), bj = pair_bj(B, p);
    const int i = 4 * r + (lane >> 4), j = lane & 15;
    const int ka = 16 * bi + i, kb = 16 * bj + j;
    if (ka >= D || kb >= D || (bi == bj && i > j)) return;
    partials[gram_index(ka, kb, D) * pstride + slot] = v;
}

// After the last tile: with split k-steps the waves' sums added in wave order (through the LDS the tiles used), then
// stored.
template <int B>
__device__ __forceinline__ void flush(f64x4 (&acc)[GramGeom<B>::NPW], double* tile, int D, int wave, int lane,
                                      double* partials, int64_t pstride, int64_t slot) {
    using G = GramGeom<B>;
    if constexpr (!G::kSplit) {
#pragma unroll
        for (int q = 0; q < G::NPW; ++q) {
            const int p = wave + q * kGramWaves;
            if (p >= G::NP) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) store_entry<B>(D, p, r, lane, acc[q][r], partials, pstride, slot);
        }
    } else {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < G::NP; ++p)
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[((wave * G::NP + p) * 4 + r) * 64 + lane] = acc[p][r];
        __syncthreads();
        for (int o = threadIdx.x; o < G::NP * 256; o += kGramThreads) {
            double v = tile[o];
            for (int w = 1; w < kGramWaves; ++w) v += tile[w * G::NP * 256 + o];
            store_entry<B>(D, o >> 8, (o >> 6) & 3, o & 63, v, partials, pstride, slot);
        }
    }
}

// The clients' pointers in LDS (a lane picks its client by a per-lane index, which the kernel-argument table cannot
// serve), and zeros in the whole tile: the rows of dead clients stay zero.
__device__ __forceinline__ void stage_init(const ClientTable& t, int D, const void** ptrs, double* tile) {
    for (int k = 0; k < D; ++k)  // k is uniform: scalar loads from the kernel arguments
        if (threadIdx.x == 0) ptrs[k] = t.src[k];
    for (int i = threadIdx.x; i < kGramLdsDoubles; i += kGramThreads) tile[i] = 0.0;
    __syncthreads();
}

// Vector form: vector v of a bucket is elements head + V v .. + V - 1, 16-byte aligned in every client and in ref.
// Tile `tl` is vectors [tl E / V, + E / V) of every client; item i of a tile is vector i % EV of client i / EV, lane
// t holding items t, t + 256, ...  The loads of the workgroup's next tile are issued before the MFMAs of this one.
template <typename T, int B>
__global__ __launch_bounds__(kGramThreads) void gram_vec_kernel(const ClientTable t, int D, const float* ref, int64_t head,
                                                                 int64_t nvec, double* partials, int64_t pstride) {
    using G = GramGeom<B>;
    constexpr int V = In<T>::kVec, EV = G::E / V, U = (16 * B * EV + kGramThreads - 1) / kGramThreads;
    __shared__ __attribute__((aligned(16))) double tile[kGramLdsDoubles];
    __shared__ const void* ptrs[kMaxClients];
    stage_init(t, D, ptrs, tile);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    f64x4 acc[G::NPW];
#pragma unroll
    for (int q = 0; q < G::NPW; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int total = D * EV;
    const int64_t ntiles = (nvec + EV - 1) / EV;
    u32x4 x[U];
    f32x4 rf[U][V / 4];
    const auto load = [&](int64_t tl) {
        const int64_t v0 = tl * EV;
        const int live = nvec - v0 < EV ? (int)(nvec - v0) : EV;  // vectors of a client in this tile
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = threadIdx.x + u * kGramThreads;
            const int k = i / EV, v = i % EV;
            x[u] = u32x4{};
            if (i >= total || v >= live) continue;
            x[u] = ld16<true>(reinterpret_cast<const T*>(ptrs[k]) + head + (v0 + v) * V);
            if (ref)
#pragma unroll
                for (int j = 0; j < V / 4; ++j) rf[u][j] = *reinterpret_cast<const f32x4*>(ref + head + (v0 + v) * V + 4 * j);
        }
    };
    int64_t tl = blockIdx.x;
    if (tl < ntiles) load(tl);
    for (; tl < ntiles; tl += gridDim.x) {
        const int64_t v0 = tl * EV;
        const int live = nvec - v0 < EV ? (int)(nvec - v0) : EV;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = threadIdx.x + u * kGramThreads;
            if (i >= total) continue;
            const int k = i / EV, v = i % EV;
            float y[V];
            In<T>::widen(x[u], y);
            if (ref && v < live)  // a dead vector stays zeros
#pragma unroll
                for (int j = 0; j < V; ++j) y[j] = y[j] - rf[u][j / 4][j % 4];
            double* dst = tile + k * G::RS + v * V;
#pragma unroll
            for (int j = 0; j < V; j += 2) *reinterpret_cast<f64x2*>(dst + j) = f64x2{(double)y[j], (double)y[j + 1]};
        }
        __syncthreads();
        if (tl + gridDim.x < ntiles) load(tl + gridDim.x);
        accumulate<B>(acc, tile, live * (V / 4), wave, lane);
        __syncthreads();
    }
    flush<B>(acc, tile, D, wave, lane, partials, pstride, blockIdx.x);
}

// Element form over elements [0, head) and [tail0, n) (the whole array: head = tail0 = n), one element per lane and
// load; its partials go to slots slot0 + blockIdx.x.
template <typename T, int B>
__global__ __launch_bounds__(kGramThreads) void gram_elem_kernel(const ClientTable t, int D, const float* ref, int64_t head,
                                                                  int64_t tail0, int64_t n, double* partials, int64_t pstride,
                                                                  int64_t slot0) {
    using G = GramGeom<B>;
    __shared__ __attribute__((aligned(16))) double tile[kGramLdsDoubles];
    __shared__ const void* ptrs[kMaxClients];
    stage_init(t, D, ptrs, tile);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    f64x4 acc[G::NPW];
#pragma unroll
    for (int q = 0; q < G::NPW; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int64_t cnt = head + (n - tail0);
    const int total = D * G::E;
    const int64_t ntiles = (cnt + G::E - 1) / G::E;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int64_t s0 = tl * G::E;
        const int live = cnt - s0 < G::E ? (int)(cnt - s0) : G::E;
        const int fill = (live + 3) / 4 * 4;  // what accumulate reads of a row
        for (int i = threadIdx.x; i < total; i += kGramThreads) {
            const int k = i / G::E, e = i % G::E;
            if (e >= fill) continue;
            float y = 0.0f;
            if (e < live) {
                const int64_t s = s0 + e, idx = s < head ? s : tail0 + (s - head);
                y = In<T>::scalar(ptrs[k], idx);
                if (ref) y = y - ref[idx];
            }
            tile[k * G::RS + e] = (double)y;
        }
        __syncthreads();
        accumulate<B>(acc, tile, fill / 4, wave, lane);
        __syncthreads();
    }
    flush<B>(acc, tile, D, wave, lane, partials, pstride, slot0 + blockIdx.x);
}

// One wave per entry a <= b: gram[a][b] = gram[b][a] = the entry's np partials, lane l adding l, l + 64, ... in
// ascending order.
__global__ __launch_bounds__(64) void gram_finish_kernel(const double* partials, int64_t pstride, int64_t np, int D,
                                                         double* gram) {
    int a = 0, r = blockIdx.x;
    while (r >= D - a) {
        r -= D - a;
        ++a;
    }
    const int b = a + r;
    const double* p = partials + (int64_t)blockIdx.x * pstride;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < np; i += 64) v += p[i];
    v = wave_sum(v);
    if (threadIdx.x == 0) {
        gram[(int64_t)a * D + b] = v;
        gram[(int64_t)b * D + a] = v;
    }
}

template <typename T, int B>
hipError_t launch_gram_t(const ClientTable& t, int D, const float* ref, const Split& sp, double* partials, double* gram,
                         const Tuning& tu, hipStream_t s) {
    const MeasureGrid gr = measure_grid(sp, GramGeom<B>::E, kGramMaxBlocks, tu.max_blocks);
    const int64_t vec_blocks = gr.vec_blocks, elem_blocks = gr.elem_blocks, np = gr.np();
    if (vec_blocks > 0) {
        hipLaunchKernelGGL((gram_vec_kernel<T, B>), dim3((unsigned)vec_blocks), dim3(kGramThreads), 0, s, t, D, ref, sp.head,
                           sp.nvec, partials, np);
        if (elem_blocks > 0)
            hipLaunchKernelGGL((gram_elem_kernel<T, B>), dim3(1), dim3(kGramThreads), 0, s, t, D, ref, sp.head, sp.tail0(),
                               sp.n, partials, np, vec_blocks);
    } else {
        hipLaunchKernelGGL((gram_elem_kernel<T, B>), dim3((unsigned)elem_blocks), dim3(kGramThreads), 0, s, t, D, ref, sp.n,
                           sp.n, sp.n, partials, np, (int64_t)0);
    }
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)gram_entries(D)), dim3(64), 0, s, partials, np, np, D, gram);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_gram_b(const ClientTable& t, int D, const float* ref, const Split& sp, double* partials, double* gram,
                         const Tuning& tu, hipStream_t s) {
    switch ((D + 15) / 16) {
        case 1: return launch_gram_t<T, 1>(t, D, ref, sp, partials, gram, tu, s);
        case 2: return launch_gram_t<T, 2>(t, D, ref, sp, partials, gram, tu, s);
        case 3: return launch_gram_t<T, 3>(t, D, ref, sp, partials, gram, tu, s);
        case 4: return launch_gram_t<T, 4>(t, D, ref, sp, partials, gram, tu, s);
        case 5: return launch_gram_t<T, 5>(t, D, ref, sp, partials, gram, tu, s);
        case 6: return launch_gram_t<T, 6>(t, D, ref, sp, partials, gram, tu, s);
        case 7: return launch_gram_t<T, 7>(t, D, ref, sp, partials, gram, tu, s);
        default: return launch_gram_t<T, 8>(t, D, ref, sp, partials, gram, tu, s);
    }
}

}  // namespace

hipError_t launch_gram(const ClientTable& t, int D, fa_dtype in, const float* ref, const Split& sp, double* partials,
                       double* gram, const Tuning& tu, hipStream_t s) {
    if (!sp.valid() || sp.V != (in == FA_F32 ? 4 : 8)) return hipErrorInvalidValue;
    if (D < 1 || D > kMaxClients || sp.n <= 0 || !gram || !partials) return hipErrorInvalidValue;
    switch (in) {
        case FA_F32: return launch_gram_b<float>(t, D, ref, sp, partials, gram, tu, s);
        case FA_BF16: return launch_gram_b<uint16_t>(t, D, ref, sp, partials, gram, tu, s);
        case FA_F16: return launch_gram_b<_Float16>(t, D, ref, sp, partials, gram, tu, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace fa
