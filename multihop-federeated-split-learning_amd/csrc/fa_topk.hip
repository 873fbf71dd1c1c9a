// fa_topk.hip -- top-k receipts (fa.h "Top-k receipts") for CDNA4 (gfx950): an update as the k (index, value) pairs of
// largest magnitude.  Two directions: the expansion of such a receipt into an ordinary slot, x = g + d with d = +0
// wherever no entry lies, and the selector that makes one from a new model and the model the owners hold.
//
// Lanes.  Both directions cut a launch into tiles of 4096 elements, one workgroup of 256 lanes per tile, lane L the 16
// consecutive elements 16 L .. 16 L + 15 of its tile.  The tiles are laid over the launch `pad` elements early, pad =
// 16 - head with head the elements before the first 16-byte boundary of the lead pointer (fa_split.h), so that every
// lane starts on a 16-byte boundary of every pointer whose phase agrees with the lead's: a lane that lies wholly inside
// the launch then moves its elements in 16-byte accesses, the lanes over the two ends (and every lane of a launch
// whose phases disagree) one element at a time with a bounds check.  One kernel serves head, vectors and tail.
//
// Expansion.  A workgroup finds the entries of its tile by two binary searches in idx, clears 16 KiB of LDS, scatters
// the values into it (ascending indices: no two entries meet in a word), and after a barrier every lane adds its 16
// LDS words to the reference and stores.  An entry is range-checked where it is applied, so unsorted input gives
// unspecified values and never a write beyond the slot.  Dense traffic: one read of g, one write of x; sparse: 8 k
// bytes.
//
// Selection: a radix select over the 31-bit magnitude keys in three histogram passes (11 + 10 + 10 bits), a counting
// pass, a scan over the tiles and a write pass -- new and sent are read five times, nothing of O(n) is kept.  A
// histogram pass counts, per workgroup in LDS, the keys whose higher digits equal the prefix found so far and merges
// its bins with integer atomics; a one-workgroup launch walks the bins from the top, appends the digit in which the
// k'-th largest key lies to the prefix, lowers the count still needed by the keys above it and clears the bins.  After
// three digits the prefix is tau and the count is the number of ties to admit.  The counting pass writes per tile the
// keys above tau and equal to tau, the scan makes them exclusive prefixes, and the write pass ranks its elements in
// index order -- per lane 16 in sequence, across lanes by a workgroup scan -- admits a tie while its rank among all
// ties is below the count, and stores the entry at (keys above before it) + min(ties before it, count): ascending
// index order, whatever the grid.  g' is stored in the same pass.  The prefix, the count and the offsets travel
// through the workspace; the host enqueues the launches back to back.  Every sum is an integer: no result depends on
// the order of the atomics.
//
// Bit-exactness: `#pragma clang fp contract(off)`; the only fp32 operations are the subtract of rule 1 and the add of
// the expansion, and the file is compiled without packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "fa_device.h"
#include "fa_host.h"
#include "fa_internal.h"
#include "fa_mx8.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kTopkThreads = 256, kTopkLane = 16, kTopkTile = kTopkTileElems;
static_assert(kTopkTile == kTopkThreads * kTopkLane, "a lane owns 16 elements of its tile");
constexpr int64_t kTopkMaxBlocks = 4096;  // 16 workgroups per CU on 256 CUs; tiles beyond it are strided
constexpr int kTopkBins = 2048;           // the widest digit: 11 bits
// The workspace, in 64-bit words: the prefix (in the end tau), the count still needed, the bins, then per tile the
// keys above tau and, `tiles` words on, the keys equal to tau.
constexpr int kWPrefix = 0, kWNeed = 1, kWHist = 2, kWTiles = kWHist + kTopkBins;

struct NoRef {};

// The lanes of one launch: n elements laid `pad` elements into the first tile; vec: a lane inside [0, n) may use
// 16-byte accesses.
struct Lanes {
    int64_t n, tiles;
    int pad, vec;
};

__device__ __forceinline__ float topk_sub(float y, float s) {
#pragma clang fp contract(off)
    return y - s;
}

template <typename T>
__device__ __forceinline__ void lane_load(const void* p, int64_t i0, bool fast, int64_t n, float* x) {
    if (fast) {
        load_ref16<T>(p, i0, x);
    } else {
#pragma unroll
        for (int j = 0; j < kTopkLane; ++j) x[j] = i0 + j >= 0 && i0 + j < n ? In<T>::scalar(p, i0 + j) : 0.0f;
    }
}
template <typename T>
__device__ __forceinline__ void lane_store(void* p, int64_t i0, bool fast, int64_t n, const float* x) {
    if (fast) {
        store16<T>(p, i0, x);
    } else {
#pragma unroll
        for (int j = 0; j < kTopkLane; ++j)
            if (i0 + j >= 0 && i0 + j < n) Out<T>::scalar(p, i0 + j, x[j]);
    }
}
// The element the calling lane starts at in tile t, and whether it takes the 16-byte form.
__device__ __forceinline__ int64_t lane_start(const Lanes& ln, int64_t t) {
    return t * kTopkTile - ln.pad + (int64_t)threadIdx.x * kTopkLane;
}
__device__ __forceinline__ bool lane_fast(const Lanes& ln, int64_t i0) {
    return ln.vec && i0 >= 0 && i0 + kTopkLane <= ln.n;
}

// ------------------------------------------------------------------ expansion

template <typename DST, typename REF>
__global__ __launch_bounds__(kTopkThreads) void topk_expand_kernel(const uint32_t* idx, const float* val, uint64_t k,
                                                                   uint64_t idx0, const void* ref, void* dst, Lanes ln) {
    __shared__ __attribute__((aligned(16))) float d[kTopkTile];
    __shared__ uint64_t rng[2];
    for (int64_t t = blockIdx.x; t < ln.tiles; t += gridDim.x) {
        const int64_t v0 = t * kTopkTile - ln.pad;  // the element of the tile's first word: < 0 in a padded first tile
        for (int j = threadIdx.x; j < kTopkTile / 4; j += kTopkThreads)
            reinterpret_cast<f32x4*>(d)[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (threadIdx.x < 2) {  // the first entry at or after the tile's first element, and after its last
            const int64_t e = threadIdx.x ? std::min<int64_t>(v0 + kTopkTile, ln.n) : std::max<int64_t>(v0, 0);
            const uint64_t target = idx0 + (uint64_t)e;
            uint64_t lo = 0, hi = k;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if ((uint64_t)idx[mid] < target) lo = mid + 1;
                else hi = mid;
            }
            rng[threadIdx.x] = lo;
        }
        __syncthreads();
        const uint64_t a = rng[0], b = rng[1];
        for (uint64_t j = a + threadIdx.x; j < b; j += kTopkThreads) {
            const uint64_t e = (uint64_t)idx[j] - idx0;  // below idx0: wraps beyond every n
            if (e >= (uint64_t)ln.n) continue;
            const int64_t pos = (int64_t)e - v0;
            if (pos >= 0 && pos < kTopkTile) d[pos] = val[j];
        }
        __syncthreads();
        const int64_t i0 = lane_start(ln, t);
        if (i0 + kTopkLane > 0 && i0 < ln.n) {
            const bool fast = lane_fast(ln, i0);
            float x[kTopkLane];
#pragma unroll
            for (int j = 0; j < kTopkLane; j += 4) {
                const f32x4 w = reinterpret_cast<const f32x4*>(d)[(threadIdx.x * kTopkLane + j) / 4];
                x[j] = w.x; x[j + 1] = w.y; x[j + 2] = w.z; x[j + 3] = w.w;
            }
            if constexpr (!__is_same(REF, NoRef)) {
                float g[kTopkLane];
                lane_load<REF>(ref, i0, fast, ln.n, g);
#pragma unroll
                for (int j = 0; j < kTopkLane; ++j) x[j] = mx8_add(g[j], x[j]);
            }
            lane_store<DST>(dst, i0, fast, ln.n, x);
        }
        __syncthreads();  // the next tile clears d
    }
}

// ------------------------------------------------------------------ selection

__device__ __forceinline__ uint32_t key_of(float d) { return __float_as_uint(d) & 0x7fffffffu; }

// The deltas of the calling lane's 16 elements of tile t (+0 outside the launch) and `sent` widened, if asked for.
template <typename T>
__device__ __forceinline__ void lane_deltas(const void* y, const void* sent, const Lanes& ln, int64_t i0, float* d,
                                            float* s) {
    const bool fast = lane_fast(ln, i0);
    lane_load<T>(y, i0, fast, ln.n, d);
    lane_load<T>(sent, i0, fast, ln.n, s);
#pragma unroll
    for (int j = 0; j < kTopkLane; ++j) d[j] = topk_sub(d[j], s[j]);
}

// The state a select starts from: no prefix, k' keys needed, empty bins; with k' = 0 a tau above every key.
__global__ __launch_bounds__(kTopkThreads) void topk_init_kernel(uint64_t* work, uint64_t kp) {
    for (int b = threadIdx.x; b < kTopkBins; b += kTopkThreads) work[kWHist + b] = 0;
    if (threadIdx.x == 0) {
        work[kWPrefix] = kp ? 0u : 0xffffffffu;
        work[kWNeed] = kp;
    }
}

// One digit's histogram: bits [shift, shift + bits) of the keys whose bits above them equal the prefix.
template <typename T>
__global__ __launch_bounds__(kTopkThreads) void topk_hist_kernel(const void* y, const void* sent, Lanes ln, uint64_t* work,
                                                                 int shift, int bits) {
    __shared__ uint32_t h[kTopkBins];
    const int nb = 1 << bits;
    for (int b = threadIdx.x; b < nb; b += kTopkThreads) h[b] = 0;
    __syncthreads();
    const uint32_t prefix = (uint32_t)work[kWPrefix];
    for (int64_t t = blockIdx.x; t < ln.tiles; t += gridDim.x) {
        const int64_t i0 = lane_start(ln, t);
        if (i0 + kTopkLane <= 0 || i0 >= ln.n) continue;
        float d[kTopkLane], s[kTopkLane];
        lane_deltas<T>(y, sent, ln, i0, d, s);
#pragma unroll
        for (int j = 0; j < kTopkLane; ++j) {
            const uint32_t key = key_of(d[j]);
            if (i0 + j >= 0 && i0 + j < ln.n && (key >> (shift + bits)) == prefix)
                atomicAdd(&h[(key >> shift) & (uint32_t)(nb - 1)], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += kTopkThreads)
        if (h[b]) atomicAdd(reinterpret_cast<unsigned long long*>(work) + kWHist + b, (unsigned long long)h[b]);
}

// The inclusive scan of v over the workgroup's 256 lanes, through s (2 x 256 words).
__device__ __forceinline__ uint64_t block_scan64(uint64_t v, uint64_t (*s)[kTopkThreads]) {
    const int t = threadIdx.x;
    int cur = 0;
    s[0][t] = v;
    __syncthreads();
    for (int o = 1; o < kTopkThreads; o <<= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= o ? s[cur][t - o] : 0);
        __syncthreads();
        cur ^= 1;
    }
    const uint64_t r = s[cur][t];
    __syncthreads();
    return r;
}

// One workgroup: the digit in which the need-th largest of the counted keys lies.  Lane t owns the bins nb - 1 -
// t per .. nb - t per - per, from the top; the lane whose bins hold the need-th key appends its digit to the prefix
// and lowers the need by the keys above it.  Every lane clears its bins for the next pass.
__global__ __launch_bounds__(kTopkThreads) void topk_digit_kernel(uint64_t* work, int bits) {
    __shared__ uint64_t s[2][kTopkThreads];
    const int per = (1 << bits) / kTopkThreads, top = (1 << bits) - 1 - (int)threadIdx.x * per;
    const uint64_t need = work[kWNeed], prefix = work[kWPrefix];
    uint64_t c[kTopkBins / kTopkThreads], sum = 0;
    for (int j = 0; j < per; ++j) {
        c[j] = work[kWHist + top - j];
        sum += c[j];
        work[kWHist + top - j] = 0;
    }
    const uint64_t incl = block_scan64(sum, s);  // also: every lane has read the state before one writes it
    uint64_t above = incl - sum;
    if (above < need && need <= incl) {
        int j = 0;
        while (above + c[j] < need) above += c[j++];
        work[kWPrefix] = prefix << bits | (uint64_t)(top - j);
        work[kWNeed] = need - above;
    }
}

// A lane's packed counts: the keys above tau in the low half, the keys equal to tau in the high half (<= 16 each; a
// tile's sums <= 4096).
__device__ __forceinline__ uint32_t lane_counts(const float* d, int64_t i0, int64_t n, uint32_t tau) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kTopkLane; ++j) {
        const uint32_t key = key_of(d[j]);
        if (i0 + j >= 0 && i0 + j < n) c += key > tau ? 1u : key == tau ? 0x10000u : 0u;
    }
    return c;
}

// The inclusive scan of v over the workgroup's 256 lanes: within a wave by shuffles, across the four through w.
__device__ __forceinline__ uint32_t block_scan32(uint32_t v, uint32_t* w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) w[wave] = v;
    __syncthreads();
    for (int i = 0; i < wave; ++i) v += w[i];
    __syncthreads();
    return v;
}

template <typename T>
__global__ __launch_bounds__(kTopkThreads) void topk_count_kernel(const void* y, const void* sent, Lanes ln,
                                                                  uint64_t* work) {
    __shared__ uint32_t w[kTopkThreads / 64];
    const uint32_t tau = (uint32_t)work[kWPrefix];
    for (int64_t t = blockIdx.x; t < ln.tiles; t += gridDim.x) {
        const int64_t i0 = lane_start(ln, t);
        uint32_t c = 0;
        if (i0 + kTopkLane > 0 && i0 < ln.n) {
            float d[kTopkLane], s[kTopkLane];
            lane_deltas<T>(y, sent, ln, i0, d, s);
            c = lane_counts(d, i0, ln.n, tau);
        }
        const uint32_t total = block_scan32(c, w);
        if (threadIdx.x == kTopkThreads - 1) {
            work[kWTiles + t] = total & 0xffffu;
            work[kWTiles + ln.tiles + t] = total >> 16;
        }
    }
}

// One workgroup: both per-tile arrays into their exclusive prefixes, lane t the tiles [t per, t per + per).
__global__ __launch_bounds__(kTopkThreads) void topk_scan_kernel(uint64_t* work, int64_t tiles) {
    __shared__ uint64_t s[2][kTopkThreads];
    const int64_t per = (tiles + kTopkThreads - 1) / kTopkThreads;
    const int64_t lo = std::min<int64_t>(tiles, (int64_t)threadIdx.x * per), hi = std::min<int64_t>(tiles, lo + per);
    for (int r = 0; r < 2; ++r) {
        uint64_t* c = work + kWTiles + r * tiles;
        uint64_t sum = 0;
        for (int64_t i = lo; i < hi; ++i) sum += c[i];
        uint64_t run = block_scan64(sum, s) - sum;
        for (int64_t i = lo; i < hi; ++i) {
            const uint64_t v = c[i];
            c[i] = run;
            run += v;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kTopkThreads) void topk_write_kernel(const void* y, const void* sent, Lanes ln,
                                                                  const uint64_t* work, uint64_t kp, uint32_t* idx,
                                                                  float* val, void* out) {
    __shared__ uint32_t w[kTopkThreads / 64];
    const uint32_t tau = (uint32_t)work[kWPrefix];
    const uint64_t need = work[kWNeed];
    for (int64_t t = blockIdx.x; t < ln.tiles; t += gridDim.x) {
        const int64_t i0 = lane_start(ln, t);
        const bool live = i0 + kTopkLane > 0 && i0 < ln.n;
        float d[kTopkLane], s[kTopkLane];
        uint32_t c = 0;
        if (live) {
            lane_deltas<T>(y, sent, ln, i0, d, s);
            c = lane_counts(d, i0, ln.n, tau);
        }
        const uint32_t before = block_scan32(c, w) - c;
        if (!live) continue;
        uint64_t gt = 0, eq = 0;  // the keys above tau and equal to tau before the lane's next element
        if (need) {
            gt = work[kWTiles + t] + (before & 0xffffu);
            eq = work[kWTiles + ln.tiles + t] + (before >> 16);
        }
#pragma unroll
        for (int j = 0; j < kTopkLane; ++j) {
            const uint32_t key = key_of(d[j]);
            const bool in = i0 + j >= 0 && i0 + j < ln.n;
            const bool tie = in && key == tau;
            const bool take = in && (key > tau || (tie && eq < need));
            const uint64_t pos = gt + std::min(eq, need);
            if (take && pos < kp) {  // pos < k' by the counts; the test keeps a write inside idx and val whatever they say
                idx[pos] = (uint32_t)(i0 + j);
                val[pos] = d[j];
            }
            gt += in && key > tau;
            eq += tie;
            s[j] = mx8_add(s[j], take ? d[j] : 0.0f);
        }
        if (out) lane_store<T>(out, i0, lane_fast(ln, i0), ln.n, s);
    }
}

unsigned topk_blocks(int64_t tiles) { return (unsigned)std::max<int64_t>(1, std::min(tiles, kTopkMaxBlocks)); }

// The lanes over a split (topk_split): a launch whose phases agree is laid so that its lanes start at 16 bytes.
Lanes topk_lanes(const Split& sp) {
    const int pad = sp.vec && sp.lead ? kTopkLane - (int)sp.lead : 0;
    return Lanes{sp.n, (sp.n + pad + kTopkTile - 1) / kTopkTile, pad, sp.vec ? 1 : 0};
}

template <typename DST, typename REF>
void launch_expand_t(const uint32_t* idx, const float* val, uint64_t k, uint64_t idx0, const void* ref, void* dst,
                     const Lanes& ln, hipStream_t s) {
    hipLaunchKernelGGL((topk_expand_kernel<DST, REF>), dim3(topk_blocks(ln.tiles)), dim3(kTopkThreads), 0, s, idx, val, k,
                       idx0, ref, dst, ln);
}

template <typename DST>
hipError_t launch_expand_d(const uint32_t* idx, const float* val, uint64_t k, uint64_t idx0, const void* ref,
                           fa_dtype rdt, void* dst, const Lanes& ln, hipStream_t s) {
    if (!ref) {
        launch_expand_t<DST, NoRef>(idx, val, k, idx0, ref, dst, ln, s);
    } else if (rdt == FA_F32) {
        launch_expand_t<DST, float>(idx, val, k, idx0, ref, dst, ln, s);
    } else {  // a 16-bit reference: the slot's own type or an f32 slot (dtype_pair_ok)
        if constexpr (__is_same(DST, float)) {
            if (rdt == FA_BF16) launch_expand_t<DST, uint16_t>(idx, val, k, idx0, ref, dst, ln, s);
            else launch_expand_t<DST, _Float16>(idx, val, k, idx0, ref, dst, ln, s);
        } else {
            launch_expand_t<DST, DST>(idx, val, k, idx0, ref, dst, ln, s);
        }
    }
    return hipGetLastError();
}

template <typename T>
hipError_t launch_encode_t(const void* y, const void* sent, uint64_t kp, uint32_t* idx, float* val, void* out,
                           uint64_t* work, const Lanes& ln, hipStream_t s) {
    const dim3 grid(topk_blocks(ln.tiles)), block(kTopkThreads);
    hipLaunchKernelGGL(topk_init_kernel, dim3(1), block, 0, s, work, kp);
    if (kp) {
        static const int kShift[3] = {20, 10, 0}, kBits[3] = {11, 10, 10};
        for (int p = 0; p < 3; ++p) {
            hipLaunchKernelGGL((topk_hist_kernel<T>), grid, block, 0, s, y, sent, ln, work, kShift[p], kBits[p]);
            hipLaunchKernelGGL(topk_digit_kernel, dim3(1), block, 0, s, work, kBits[p]);
        }
        hipLaunchKernelGGL((topk_count_kernel<T>), grid, block, 0, s, y, sent, ln, work);
        hipLaunchKernelGGL(topk_scan_kernel, dim3(1), block, 0, s, work, ln.tiles);
    }
    if (kp || out) hipLaunchKernelGGL((topk_write_kernel<T>), grid, block, 0, s, y, sent, ln, work, kp, idx, val, out);
    return hipGetLastError();
}

}  // namespace

// The split of a launch led by `lead` (elements of `elem` bytes): the head brings it to 16 bytes, a vector is a
// lane's 16 elements.  Every other pointer is required after the same head (Split::require).
Split topk_split(const void* lead, size_t elem, size_t n) {
    Split sp = split_at(lead, elem, n);
    sp.nvec = ((int64_t)n - sp.head) / kTopkLane;
    sp.V = kTopkLane;
    return sp;
}

size_t topk_workspace(size_t n) {
    return ((size_t)kWTiles + 2 * ((n + kTopkLane - 1) / kTopkTile + 1)) * sizeof(uint64_t);
}

hipError_t launch_topk_expand(const uint32_t* idx, const float* val, uint64_t k, uint64_t idx0, int64_t n, const void* ref,
                              fa_dtype rdt, void* dst, fa_dtype ddt, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if ((k && (!idx || !val)) || !dst || (ref && !dtype_pair_ok(ddt, rdt))) return hipErrorInvalidValue;
    Split sp = topk_split(dst, ddt == FA_F32 ? 4 : 2, (size_t)n);
    if (ref) sp.require(ref, rdt == FA_F32 ? 4 : 2);
    const Lanes ln = topk_lanes(sp);
    switch (ddt) {
        case FA_F32: return launch_expand_d<float>(idx, val, k, idx0, ref, rdt, dst, ln, s);
        case FA_BF16: return launch_expand_d<uint16_t>(idx, val, k, idx0, ref, rdt, dst, ln, s);
        case FA_F16: return launch_expand_d<_Float16>(idx, val, k, idx0, ref, rdt, dst, ln, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_topk_encode(const void* y, const void* sent, fa_dtype dt, int64_t n, uint64_t k, uint32_t* idx,
                              float* val, void* out, void* work, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const uint64_t kp = std::min<uint64_t>(k, (uint64_t)n);
    if (!y || !sent || !work || (kp && (!idx || !val))) return hipErrorInvalidValue;
    const size_t es = dt == FA_F32 ? 4 : 2;
    Split sp = topk_split(y, es, (size_t)n);
    sp.require(sent, es);
    if (out) sp.require(out, es);
    const Lanes ln = topk_lanes(sp);
    uint64_t* w = static_cast<uint64_t*>(work);
    switch (dt) {
        case FA_F32: return launch_encode_t<float>(y, sent, kp, idx, val, out, w, ln, s);
        case FA_BF16: return launch_encode_t<uint16_t>(y, sent, kp, idx, val, out, w, ln, s);
        case FA_F16: return launch_encode_t<_Float16>(y, sent, kp, idx, val, out, w, ln, s);
    }
    return hipErrorInvalidValue;
}

// Rules 2-5 on the host: tau by a partial sort of the keys, then one pass in index order.
void topk_encode_host(const float* delta, size_t n, size_t kp, uint32_t* idx, float* val) {
    if (kp == 0) return;
    const auto key = [&](size_t i) { return __builtin_bit_cast(uint32_t, delta[i]) & 0x7fffffffu; };
    std::vector<uint32_t> keys(n);
    for (size_t i = 0; i < n; ++i) keys[i] = key(i);
    std::nth_element(keys.begin(), keys.begin() + (kp - 1), keys.end(), [](uint32_t a, uint32_t b) { return a > b; });
    const uint32_t tau = keys[kp - 1];
    size_t above = 0;
    for (size_t i = 0; i < n; ++i) above += key(i) > tau;
    size_t need = kp - above, j = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t ki = key(i);
        if (!(ki > tau || (ki == tau && need))) continue;
        if (ki == tau) --need;
        idx[j] = (uint32_t)i;
        val[j++] = delta[i];
    }
}

}  // namespace fa

using namespace fah;

extern "C" {

int fa_topk_encode(const float* delta, size_t n, size_t k, uint32_t* idx, float* val, size_t* k_out) {
    g_err.clear();
    const size_t kp = std::min(k, n);
    if ((uint64_t)n > (1ull << 32) && kp) return fail(FA_ERR_ARG, "topk: a bucket with entries holds at most 2^32 elements");
    if (k_out) *k_out = kp;
    if (kp == 0) return FA_OK;
    if (!delta || !idx || !val) return fail(FA_ERR_ARG, "topk: %s is null", !delta ? "delta" : !idx ? "idx" : "val");
    fa::topk_encode_host(delta, n, kp, idx, val);
    return FA_OK;
}

int fa_topk_decode(const uint32_t* idx, const float* val, size_t k, uint64_t idx0, size_t n, float* d) {
    g_err.clear();
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "topk: idx0 + n beyond 2^64");
    if (k && (!idx || !val)) return fail(FA_ERR_ARG, "topk: %s is null", !idx ? "idx" : "val");
    for (size_t j = 1; j < k; ++j)
        if (idx[j] <= idx[j - 1])
            return fail(FA_ERR_ARG, "topk: idx[%zu] = %u after idx[%zu] = %u: not strictly ascending", j, idx[j], j - 1, idx[j - 1]);
    if (n == 0) return FA_OK;
    if (!d) return fail(FA_ERR_ARG, "topk: d is null");
    std::fill(d, d + n, 0.0f);
    for (size_t j = 0; j < k; ++j)
        if ((uint64_t)idx[j] >= idx0 && (uint64_t)idx[j] - idx0 < (uint64_t)n) d[(uint64_t)idx[j] - idx0] = val[j];
    return FA_OK;
}

int fa_topk_expand_device(fa_ctx* ctx, int gpu, const uint32_t* d_idx, const float* d_val, size_t k, size_t n,
                          uint64_t idx0, const void* d_ref, fa_dtype ref_dtype, void* d_dst, fa_dtype dst_dtype,
                          void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!dvalid(dst_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (!fa::dtype_pair_ok(dst_dtype, ref_dtype))
        return fail(FA_ERR_ARG, "topk: no %s slot against a %s reference (a 16-bit slot takes its own type or f32)",
                    fa::dtype_name(dst_dtype), fa::dtype_name(ref_dtype));
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "topk: idx0 + n beyond 2^64");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if ((k && (!d_idx || !d_val)) || !d_dst)
        return fail(FA_ERR_ARG, "topk: %s pointer is null", !d_dst ? "d_dst" : !d_idx ? "d_idx" : "d_val");
    if (!aligned(d_idx, 4) || !aligned(d_val, 4)) return fail(FA_ERR_ALIGN, "topk: %s not 4-byte aligned", !aligned(d_idx, 4) ? "d_idx" : "d_val");
    if (d_ref && !aligned(d_ref, dsize(ref_dtype)))
        return fail(FA_ERR_ALIGN, "topk: reference not %zu-byte aligned", dsize(ref_dtype));
    if (!aligned(d_dst, dsize(dst_dtype))) return fail(FA_ERR_ALIGN, "topk: slot not %zu-byte aligned", dsize(dst_dtype));
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_topk_expand(d_idx, d_val, k, idx0, (int64_t)n, d_ref, ref_dtype, d_dst, dst_dtype, c.s));
    return FA_OK;
}

size_t fa_topk_encode_workspace(size_t n) { return fa::topk_workspace(n); }

int fa_topk_encode_device(fa_ctx* ctx, int gpu, const void* d_new, fa_dtype new_dtype, const void* d_sent,
                          fa_dtype sent_dtype, size_t n, size_t k, uint32_t* d_idx, float* d_val, void* d_out,
                          void* d_work, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!dvalid(new_dtype) || !dvalid(sent_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (new_dtype != sent_dtype)
        return fail(FA_ERR_ARG, "topk: the new model is %s, the sent one %s: one dtype", fa::dtype_name(new_dtype),
                    fa::dtype_name(sent_dtype));
    if (k && (uint64_t)n > (1ull << 32)) return fail(FA_ERR_ARG, "topk: a bucket with entries holds at most 2^32 elements");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if (!d_new || !d_sent || !d_work || (k && (!d_idx || !d_val)))
        return fail(FA_ERR_ARG, "topk: %s pointer is null", !d_new ? "d_new" : !d_sent ? "d_sent" : !d_work ? "d_work" : !d_idx ? "d_idx" : "d_val");
    const size_t es = dsize(new_dtype);
    if (!aligned(d_new, es) || !aligned(d_sent, es) || (d_out && !aligned(d_out, es)))
        return fail(FA_ERR_ALIGN, "topk: %s not %zu-byte aligned", !aligned(d_new, es) ? "d_new" : !aligned(d_sent, es) ? "d_sent" : "d_out", es);
    if (!aligned(d_idx, 4) || !aligned(d_val, 4) || !aligned(d_work, 16))
        return fail(FA_ERR_ALIGN, "topk: %s not aligned", !aligned(d_idx, 4) ? "d_idx" : !aligned(d_val, 4) ? "d_val" : "d_work (16 bytes)");
    if (d_out) {  // the same address as an input, or apart from it
        const uintptr_t o = (uintptr_t)d_out, bytes = (uintptr_t)(n * es);
        for (const void* in : {d_new, d_sent}) {
            const uintptr_t a = (uintptr_t)in;
            if (o != a && o < a + bytes && a < o + bytes)
                return fail(FA_ERR_ARG, "topk: d_out overlaps %s without being it", in == d_new ? "d_new" : "d_sent");
        }
    }
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_topk_encode(d_new, d_sent, new_dtype, (int64_t)n, (uint64_t)k, d_idx, d_val, d_out, d_work, c.s));
    return FA_OK;
}

}  // extern "C"
