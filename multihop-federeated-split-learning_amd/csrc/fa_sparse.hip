// fa_sparse.hip -- the sparse-sum stage (fa.h "Sparse-sum stage") for CDNA4 (gfx950): the top-k receipts of a round
// reduced straight from their (idx, val) arrays into the fp32 aggregate, a_i = g_i + sum_c w_c d_c,i, without ever
// expanding a receipt into a dense slot.  The sum of an element is a chain of fused multiply-adds in ascending client
// order over the clients that named it: no floating-point atomics, the same bits for every grid, tile size and phase.
//
// Two passes per launch.
//
// Cut pass.  Tiles of E elements are laid over the launch (`pad` elements early, as fa_topk.hip lays its tiles, so
// that a lane of the dense side starts on a 16-byte boundary of g and the output).  One streaming pass over every
// client's idx writes the table T[t D + c] = the first entry of client c at or after tile t, t = 0 .. tiles: the lane
// of entry j (and of the end, j = k) compares the tile of idx[j] with that of idx[j - 1] and writes j for every tile
// in between, so empty tiles are covered without a clear; a client with no entries has its column written by all its
// lanes.  Entries below the launch come before tile 0, entries at or beyond its end after the last tile.  Whatever
// idx holds, every word of T is written (a walk from -1 to `tiles` crosses every tile) and every word is <= k.  The
// table is tile-major: the accumulate pass reads the 2 D words of a tile in two coalesced loads.  It replaces 2 D
// dependent binary searches per tile by coalesced reads of 4 sum k bytes.
//
// Accumulate pass: one wave per tile, one wave per workgroup, no barrier anywhere.  The wave owns E fp32 accumulators
// in LDS, cleared first.  Lane c (and c + 64) holds the bounds of client c in registers; a wave-uniform v_readlane
// hands them out, so the client loop waits for no table load.  For c = 0 .. D - 1 lane l takes entry lo_c + l, then
// + 64 and so on: it reads its accumulator word, does fmaf(w_c, val, acc) and writes it back.  One client's indices
// are distinct, so no two lanes of an instruction meet in a word; LDS serves one wave's instructions in order, so
// client c + 1 sees what client c wrote (a wavefront-scope fence keeps the compiler from moving an access across
// it; it costs no instruction).  The first 64 entries of the next kGroup = 4 clients are loaded while the current
// group is applied; entries beyond a client's first 64 in a tile are loaded where they are applied (a deviation
// from "everything in flight": at the densities where a client has more than 64 entries per tile the lanes are
// full and the wave's neighbours hide the latency).  Every entry is range-checked against the launch and the tile
// where it is applied: unsorted input gives unspecified values, never an access outside the accumulators, and the
// bounds never exceed k.  Then the dense side: per round of 1024 elements a lane reads 16 accumulator words as four
// 16-byte LDS reads, adds g (one IEEE add, also where nobody named the element: -0 + +0 = +0) and stores, in 16-byte
// accesses where the lane lies inside the launch and the phases of g and the output agree (fa_split.h), else element
// by element with a bounds check.  A workgroup-wide tile would need D barriers per tile and keep about 40 of 256
// lanes busy between them at 1 % density; the wave-wide tile needs none.
//
// The client table -- idx, val, k and w of up to 128 clients, 3 KiB -- travels in the kernel-argument segment (4 KiB):
// no upload, no dependence on the caller's host memory after the call returns, and every access to it is a scalar
// load with a wave-uniform index.  That is why k_c <= 2^32 - 1: a count fits the table's 32-bit words.
//
// Tile size is a form.  Lane use per client is rho E / 64 for density rho, LDS per wave 4 E bytes.  E = 2048 (8 KiB,
// 5 waves per SIMD by LDS) or E = 8192 (32 KiB, 5 waves per CU), chosen on the host from sum k / (D n)
// (sparse_tile_form).  Measured: the small tile wins at every density from 1 / 1000 to 1 / 10 -- by 7 % at
// 1 / 1000, by 2.3 times at 1 / 10 -- although it fills a third of a wave per client at 1 / 100: occupancy hides the
// latency of the dependent LDS chain better than fuller instructions do.  The big tile is kept for densities below
// 1 / 2048, less than one entry per client and small tile, where a tile's 8 D bytes of table outweigh its entries and
// the big tile reads a quarter of them; that region has not been measured.
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950): the accumulate kernels take 44 - 56 VGPRs in every
// dtype pair (absolute mode 44 - 53), 0 AGPRs, no scratch, no spills; LDS 8192 bytes and 5 waves per SIMD at E = 2048,
// 32768 bytes and 2 waves per SIMD (5 workgroups of one wave per CU) at E = 8192.  The cut kernel: 14 VGPRs, no LDS, no
// scratch, 8 waves per SIMD.
//
// Bit-exactness: `#pragma clang fp contract(off)`; the fp32 operations are the fused multiply-add of rule 1 (written
// as one) and the add of rule 2, and the file is compiled without packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "fa_device.h"
#include "fa_host.h"
#include "fa_internal.h"
#include "fa_mx8.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kLane = 16;             // the elements a lane moves at once on the dense side
constexpr int kRound = 64 * kLane;    // the elements a wave moves per round of the dense side
constexpr int kGroup = kSparseGroup;  // the clients whose first entries are in flight
constexpr int kCutThreads = 256;
constexpr int64_t kCutMaxBlocks = 1024;  // per client; entries beyond it are strided
static_assert(kSparseTileSmall % kRound == 0 && kSparseTileBig % kRound == 0, "a tile is whole rounds");

struct NoRef {};

struct SparseTable {  // 3 KiB of the kernel-argument segment
    const uint32_t* idx[kMaxClients];
    const float* val[kMaxClients];
    uint32_t k[kMaxClients];
    float w[kMaxClients];
};

// One launch: n elements, bucket elements idx0 .., laid `pad` elements into the first of `tiles` tiles of 1 << shift
// elements; vec: a lane inside [0, n) may use 16-byte accesses.
struct SparseLanes {
    int64_t n, tiles;
    uint64_t idx0;
    int pad, vec, shift, D;
};

// The tile an entry belongs to: -1 below the launch, `tiles` beyond its last tile.
__device__ __forceinline__ int64_t tile_of(uint32_t i, const SparseLanes& ln) {
    if ((uint64_t)i < ln.idx0) return -1;
    const uint64_t q = ((uint64_t)i - ln.idx0 + (uint64_t)ln.pad) >> ln.shift;
    return q < (uint64_t)ln.tiles ? (int64_t)q : ln.tiles;
}

__global__ __launch_bounds__(kCutThreads) void sparse_cut_kernel(const SparseTable tb, const SparseLanes ln, uint32_t* tab) {
    const int c = (int)blockIdx.y;
    const uint32_t* idx = tb.idx[c];
    const uint64_t k = tb.k[c];
    const uint64_t stride = (uint64_t)gridDim.x * kCutThreads;
    const uint64_t tid = (uint64_t)blockIdx.x * kCutThreads + threadIdx.x;
    if (k == 0) {  // wave-uniform: no entry walks the tiles, so every lane writes its share of the column
        for (uint64_t t = tid; t <= (uint64_t)ln.tiles; t += stride) tab[t * (uint64_t)ln.D + c] = 0u;
        return;
    }
    for (uint64_t j = tid; j <= k; j += stride) {
        const int64_t prev = j ? tile_of(idx[j - 1], ln) : -1;
        const int64_t cur = j < k ? tile_of(idx[j], ln) : ln.tiles;
        for (int64_t t = prev + 1; t <= cur; ++t) tab[t * ln.D + c] = (uint32_t)j;
    }
}

__device__ __forceinline__ float sparse_fma(float w, float d, float acc) { return __builtin_fmaf(w, d, acc); }

// What one client wrote is what the next one reads: the order of a wave's LDS instructions does the rest.
__device__ __forceinline__ void wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__device__ __forceinline__ void lane_load(const void* p, int64_t i0, bool fast, int64_t n, float* x) {
    if (fast) {
        load_ref16<T>(p, i0, x);
    } else {
#pragma unroll
        for (int j = 0; j < kLane; ++j) x[j] = i0 + j >= 0 && i0 + j < n ? In<T>::scalar(p, i0 + j) : 0.0f;
    }
}
template <typename T>
__device__ __forceinline__ void lane_store(void* p, int64_t i0, bool fast, int64_t n, const float* x) {
    if (fast) {
        store16<T>(p, i0, x);
    } else {
#pragma unroll
        for (int j = 0; j < kLane; ++j)
            if (i0 + j >= 0 && i0 + j < n) Out<T>::scalar(p, i0 + j, x[j]);
    }
}

struct Chunk {  // a lane's entry of each client of a group
    uint32_t i[kGroup];
    float v[kGroup];
};

template <int E, typename DST, typename REF>
__global__ __launch_bounds__(64) void sparse_sum_kernel(const SparseTable tb, const SparseLanes ln, const uint32_t* tab,
                                                        const void* ref, void* dst) {
    __shared__ __attribute__((aligned(16))) float acc[E];
    const int lane = (int)threadIdx.x, D = ln.D;
    for (int64_t t = blockIdx.x; t < ln.tiles; t += gridDim.x) {
        const int64_t v0 = t * E - ln.pad;  // the element of the tile's first word: < 0 in a padded first tile
#pragma unroll 4
        for (int j = lane; j < E / 4; j += 64) reinterpret_cast<f32x4*>(acc)[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // the bounds of client `lane` and client `lane + 64` in this tile
        const uint32_t* row = tab + t * D;
        const int lo0 = lane < D ? (int)row[lane] : 0, hi0 = lane < D ? (int)row[D + lane] : 0;
        const int lo1 = lane + 64 < D ? (int)row[lane + 64] : 0, hi1 = lane + 64 < D ? (int)row[D + lane + 64] : 0;
        const auto bounds = [&](int c, uint64_t& lo, uint64_t& hi) {  // c wave-uniform
            lo = (uint32_t)__builtin_amdgcn_readlane(c < 64 ? lo0 : lo1, c & 63);
            hi = (uint32_t)__builtin_amdgcn_readlane(c < 64 ? hi0 : hi1, c & 63);
        };
        const auto fetch = [&](int c0, Chunk& ch) {
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const int c = c0 + u;
                ch.i[u] = 0u;
                ch.v[u] = 0.0f;
                if (c < D) {
                    uint64_t lo, hi;
                    bounds(c, lo, hi);
                    const uint64_t j = lo + (uint64_t)lane;
                    if (j < hi) {
                        ch.i[u] = tb.idx[c][j];
                        ch.v[u] = tb.val[c][j];
                    }
                }
            }
        };
        const auto apply = [&](uint32_t i, float d, float w) {
            const uint64_t e = (uint64_t)i - ln.idx0;  // below idx0: wraps beyond every n
            if (e >= (uint64_t)ln.n) return;
            const int64_t pos = (int64_t)e - v0;
            if (pos >= 0 && pos < E) acc[pos] = sparse_fma(w, d, acc[pos]);
        };
        Chunk cur;
        fetch(0, cur);
        wave_order();  // the clear
        for (int c0 = 0; c0 < D; c0 += kGroup) {
            Chunk nxt;
            fetch(c0 + kGroup, nxt);
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const int c = c0 + u;
                if (c < D) {  // wave-uniform
                    uint64_t lo, hi;
                    bounds(c, lo, hi);
                    const float w = tb.w[c];
                    uint64_t j = lo + (uint64_t)lane;
                    if (j < hi) apply(cur.i[u], cur.v[u], w);
                    for (j += 64; j < hi; j += 64) apply(tb.idx[c][j], tb.val[c][j], w);
                    wave_order();
                }
            }
            cur = nxt;
        }
        // the dense side
#pragma unroll 2
        for (int r = 0; r < E / kRound; ++r) {
            const int at = r * kRound + lane * kLane;
            const int64_t i0 = v0 + at;
            if (i0 + kLane > 0 && i0 < ln.n) {
                const bool fast = ln.vec && i0 >= 0 && i0 + kLane <= ln.n;
                float x[kLane];
#pragma unroll
                for (int j = 0; j < kLane; j += 4) {
                    const f32x4 q = reinterpret_cast<const f32x4*>(acc)[(at + j) / 4];
                    x[j] = q.x; x[j + 1] = q.y; x[j + 2] = q.z; x[j + 3] = q.w;
                }
                if constexpr (!__is_same(REF, NoRef)) {
                    float g[kLane];
                    lane_load<REF>(ref, i0, fast, ln.n, g);
#pragma unroll
                    for (int j = 0; j < kLane; ++j) x[j] = mx8_add(g[j], x[j]);
                }
                lane_store<DST>(dst, i0, fast, ln.n, x);
            }
        }
        wave_order();  // the next tile clears acc
    }
}

template <int E, typename DST, typename REF>
void launch_sum_t(const SparseTable& tb, const SparseLanes& ln, const uint32_t* tab, const void* ref, void* dst,
                  int64_t cap, hipStream_t s) {
    hipLaunchKernelGGL((sparse_sum_kernel<E, DST, REF>), dim3((unsigned)std::max<int64_t>(1, std::min(ln.tiles, cap))),
                       dim3(64), 0, s, tb, ln, tab, ref, dst);
}

template <int E, typename DST>
void launch_sum_d(const SparseTable& tb, const SparseLanes& ln, const uint32_t* tab, const void* ref, fa_dtype rdt,
                  void* dst, int64_t cap, hipStream_t s) {
    if (!ref) {
        launch_sum_t<E, DST, NoRef>(tb, ln, tab, ref, dst, cap, s);
    } else if (rdt == FA_F32) {
        launch_sum_t<E, DST, float>(tb, ln, tab, ref, dst, cap, s);
    } else {  // a 16-bit reference: the output's own type or an f32 output (dtype_pair_ok)
        if constexpr (__is_same(DST, float)) {
            if (rdt == FA_BF16) launch_sum_t<E, DST, uint16_t>(tb, ln, tab, ref, dst, cap, s);
            else launch_sum_t<E, DST, _Float16>(tb, ln, tab, ref, dst, cap, s);
        } else {
            launch_sum_t<E, DST, DST>(tb, ln, tab, ref, dst, cap, s);
        }
    }
}

template <int E>
void launch_sum_e(const SparseTable& tb, const SparseLanes& ln, const uint32_t* tab, const void* ref, fa_dtype rdt,
                  void* dst, fa_dtype ddt, int64_t cap, hipStream_t s) {
    switch (ddt) {
        case FA_F32: return launch_sum_d<E, float>(tb, ln, tab, ref, rdt, dst, cap, s);
        case FA_BF16: return launch_sum_d<E, uint16_t>(tb, ln, tab, ref, rdt, dst, cap, s);
        case FA_F16: return launch_sum_d<E, _Float16>(tb, ln, tab, ref, rdt, dst, cap, s);
    }
}

// The lanes of a launch in tile form `form`: the split is led by the output, as the expansion's by its slot.
SparseLanes sparse_lanes(size_t n, uint64_t idx0, int D, const void* ref, fa_dtype rdt, const void* out, fa_dtype odt,
                         int form) {
    Split sp = topk_split(out, odt == FA_F32 ? 4 : 2, n);
    if (ref) sp.require(ref, rdt == FA_F32 ? 4 : 2);
    const int pad = sp.vec && sp.lead ? kLane - (int)sp.lead : 0;
    const int shift = form == kSparseBig ? 13 : 11;
    static_assert(kSparseTileSmall == 1 << 11 && kSparseTileBig == 1 << 13, "the shifts of the two tiles");
    return SparseLanes{(int64_t)n, (int64_t)(((uint64_t)n + (uint64_t)pad + ((1u << shift) - 1)) >> shift), idx0, pad,
                       sp.vec ? 1 : 0, shift, D};
}

}  // namespace

int sparse_tile_form(const uint64_t* k, int D, size_t n) {
    uint64_t sum = 0;  // <= 128 (2^32 - 1): 2048 sum < 2^51, and an n beyond 2^55 decides by itself
    for (int c = 0; c < D; ++c) sum += k[c];
    return sum * kSparseTileSmall < (uint64_t)D * std::min<uint64_t>(n, 1ull << 55) ? kSparseBig : kSparseSmall;
}

bool sparse_vec(size_t n, const void* ref, fa_dtype rdt, const void* out, fa_dtype odt) {
    return sparse_lanes(n, 0, 1, ref, rdt, out, odt, kSparseSmall).vec != 0;
}

// D columns of (tiles + 1) words at the small tile, a padded first tile included.
size_t sparse_workspace(size_t n, int D) {
    const size_t tiles = (n + (size_t)kLane + kSparseTileSmall - 1) / kSparseTileSmall;
    return ((size_t)std::max(D, 0) * (tiles + 1) * sizeof(uint32_t) + 15) / 16 * 16;
}

hipError_t launch_sparse_sum(const uint32_t* const* idx, const float* const* val, const uint64_t* k, const float* w, int D,
                             uint64_t idx0, int64_t n, const void* ref, fa_dtype rdt, void* out, fa_dtype odt, void* work,
                             int form, const Tuning& tu, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (D < 1 || D > kMaxClients || !idx || !val || !k || !w || !out || !work || (ref && !dtype_pair_ok(rdt, odt)))
        return hipErrorInvalidValue;
    SparseTable tb;
    uint64_t kmax = 0;
    for (int c = 0; c < kMaxClients; ++c) {
        const bool in = c < D;
        if (in && (k[c] > 0xffffffffull || (k[c] && (!idx[c] || !val[c])))) return hipErrorInvalidValue;
        tb.idx[c] = in ? idx[c] : nullptr;
        tb.val[c] = in ? val[c] : nullptr;
        tb.k[c] = in ? (uint32_t)k[c] : 0u;
        tb.w[c] = in ? w[c] : 0.0f;
        if (in) kmax = std::max(kmax, k[c]);
    }
    if (form != kSparseSmall && form != kSparseBig) form = sparse_tile_form(k, D, (size_t)n);
    const SparseLanes ln = sparse_lanes((size_t)n, idx0, D, ref, rdt, out, odt, form);
    uint32_t* tab = static_cast<uint32_t*>(work);
    const int64_t cut_blocks = std::max<int64_t>(1, std::min<int64_t>((int64_t)((kmax + kCutThreads) / kCutThreads), kCutMaxBlocks));
    hipLaunchKernelGGL(sparse_cut_kernel, dim3((unsigned)cut_blocks, (unsigned)D), dim3(kCutThreads), 0, s, tb, ln, tab);
    // a wave per workgroup: 16 (8 KiB of LDS) or 4 (32 KiB) per CU on 256 CUs; tiles beyond it are strided.  The 20 and
    // 5 that the LDS would hold took about 1.2 times as long in a run whose data was not kept
    int64_t cap = form == kSparseBig ? 1024 : 4096;
    if (tu.max_blocks > 0) cap = std::min<int64_t>(cap, tu.max_blocks);
    if (form == kSparseBig) launch_sum_e<kSparseTileBig>(tb, ln, tab, ref, rdt, out, odt, cap, s);
    else launch_sum_e<kSparseTileSmall>(tb, ln, tab, ref, rdt, out, odt, cap, s);
    return hipGetLastError();
}

// Rules 1-2 on the host: client by client, which is every element's chain in ascending client order.
void sparse_sum_host(const uint32_t* const* idx, const float* const* val, const uint64_t* k, const float* w, int D, size_t n,
                     uint64_t idx0, const float* ref, float* out) {
#pragma clang fp contract(off)
    std::fill(out, out + n, 0.0f);
    for (int c = 0; c < D; ++c)
        for (uint64_t j = 0; j < k[c]; ++j) {
            const uint64_t e = (uint64_t)idx[c][j] - idx0;
            if (e < (uint64_t)n) out[e] = std::fmaf(w[c], val[c][j], out[e]);
        }
    for (size_t i = 0; ref && i < n; ++i) out[i] = ref[i] + out[i];
}

}  // namespace fa

using namespace fah;

namespace {

// What fa_sparse_sum_host, fa_sparse_sum_device and fa_sparse_sum_form refuse before they look at a pointer's target;
// the counts as 64-bit words into kk.
int check_sparse_sum(const void* const* idx, const void* const* val, const size_t* k, const float* w, int D, size_t n,
                     uint64_t idx0, std::vector<uint64_t>* kk) {
    if (D < 1 || D > FA_SPARSE_MAX_CLIENTS) return fail(FA_ERR_ARG, "sparse: D = %d clients outside 1 .. %d", D, FA_SPARSE_MAX_CLIENTS);
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "sparse: idx0 + n beyond 2^64");
    if (!k) return fail(FA_ERR_ARG, "sparse: k is null");
    kk->assign(k, k + D);
    for (int c = 0; c < D; ++c) {
        if ((uint64_t)k[c] > 0xffffffffull)
            return fail(FA_ERR_ARG, "sparse: client %d has %zu entries, a receipt holds at most 2^32 - 1", c, k[c]);
        if (k[c] && idx0 + (uint64_t)n > (1ull << 32))
            return fail(FA_ERR_ARG, "sparse: a bucket with entries holds at most 2^32 elements");
    }
    if (n == 0) return FA_OK;
    if (!idx || !val || !w) return fail(FA_ERR_ARG, "sparse: %s is null", !idx ? "idx" : !val ? "val" : "w");
    for (int c = 0; c < D; ++c) {
        if (k[c] && (!idx[c] || !val[c])) return fail(FA_ERR_ARG, "sparse: client %d's %s is null", c, !idx[c] ? "idx" : "val");
        if (!aligned(idx[c], 4) || !aligned(val[c], 4))
            return fail(FA_ERR_ALIGN, "sparse: client %d's %s not 4-byte aligned", c, !aligned(idx[c], 4) ? "idx" : "val");
    }
    return FA_OK;
}

// The operands of the dense side.
int check_sparse_dense(size_t n, const void* d_ref, fa_dtype rdt, const void* d_out, fa_dtype odt) {
    if (!d_out) return fail(FA_ERR_ARG, "sparse: d_out is null");
    if (d_ref && !aligned(d_ref, dsize(rdt))) return fail(FA_ERR_ALIGN, "sparse: reference not %zu-byte aligned", dsize(rdt));
    if (!aligned(d_out, dsize(odt))) return fail(FA_ERR_ALIGN, "sparse: output not %zu-byte aligned", dsize(odt));
    if (d_ref) {
        const uintptr_t o = (uintptr_t)d_out, r = (uintptr_t)d_ref;
        if (o < r + n * dsize(rdt) && r < o + n * dsize(odt)) return fail(FA_ERR_ARG, "sparse: d_out overlaps d_ref");
    }
    return FA_OK;
}

}  // namespace

extern "C" {

int fa_sparse_sum_host(const uint32_t* const* idx, const float* const* val, const size_t* k, const float* w, int D, size_t n,
                       uint64_t idx0, const float* ref, float* out) {
    g_err.clear();
    std::vector<uint64_t> kk;
    if (int rc = check_sparse_sum(reinterpret_cast<const void* const*>(idx), reinterpret_cast<const void* const*>(val), k, w, D,
                                  n, idx0, &kk))
        return rc;
    if (n == 0) return FA_OK;
    if (!out) return fail(FA_ERR_ARG, "sparse: out is null");
    fa::sparse_sum_host(idx, val, kk.data(), w, D, n, idx0, ref, out);
    return FA_OK;
}

size_t fa_sparse_sum_workspace(size_t n, int D) { return fa::sparse_workspace(n, D); }

int fa_diag_sparse_sum(fa_ctx* ctx, int gpu, const uint32_t* const* d_idx, const float* const* d_val, const size_t* k,
                       const float* w, int D, size_t n, uint64_t idx0, const void* d_ref, fa_dtype ref_dtype, void* d_out,
                       fa_dtype out_dtype, void* d_work, int form, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!dvalid(out_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    FA_PAIR(ref_dtype, out_dtype);
    std::vector<uint64_t> kk;
    if (int rc = check_sparse_sum(reinterpret_cast<const void* const*>(d_idx), reinterpret_cast<const void* const*>(d_val), k,
                                  w, D, n, idx0, &kk))
        return rc;
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if (int rc = check_sparse_dense(n, d_ref, ref_dtype, d_out, out_dtype)) return rc;
    if (!d_work) return fail(FA_ERR_ARG, "sparse: d_work is null");
    if (!aligned(d_work, 16)) return fail(FA_ERR_ALIGN, "sparse: d_work not 16-byte aligned");
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_sparse_sum(d_idx, d_val, kk.data(), w, D, idx0, (int64_t)n, d_ref, ref_dtype, d_out, out_dtype, d_work,
                                 form, c.tu, c.s));
    return FA_OK;
}

int fa_sparse_sum_device(fa_ctx* ctx, int gpu, const uint32_t* const* d_idx, const float* const* d_val, const size_t* k,
                         const float* w, int D, size_t n, uint64_t idx0, const void* d_ref, fa_dtype ref_dtype, void* d_out,
                         fa_dtype out_dtype, void* d_work, void* hip_stream) {
    return fa_diag_sparse_sum(ctx, gpu, d_idx, d_val, k, w, D, n, idx0, d_ref, ref_dtype, d_out, out_dtype, d_work, -1,
                              hip_stream);
}

int fa_sparse_sum_form(size_t n, const size_t* k, int D, const void* d_ref, fa_dtype ref_dtype, const void* d_out,
                       fa_dtype out_dtype) {
    g_err.clear();
    if (!dvalid(out_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    FA_PAIR(ref_dtype, out_dtype);
    std::vector<uint64_t> kk;
    if (int rc = check_sparse_sum(nullptr, nullptr, k, nullptr, D, 0, 0, &kk)) return rc;
    if (int rc = check_sparse_dense(0, d_ref, ref_dtype, d_out, out_dtype)) return rc;
    return (fa::sparse_vec(n, d_ref, ref_dtype, d_out, out_dtype) ? FA_SPARSE_VECTOR : 0) |
           (fa::sparse_tile_form(kk.data(), D, n) == fa::kSparseBig ? FA_SPARSE_BIG_TILE : 0);
}

}  // extern "C"
