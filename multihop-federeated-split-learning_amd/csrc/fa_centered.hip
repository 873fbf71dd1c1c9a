// fa_centered.hip -- the centred mean of the Bulyan stage (fa.h "Bulyan stage", rule 4) for CDNA4 (gfx950).
//
// Per element: the nc client values are widened, keyed and sorted exactly as in fa_trimmed.hip (fa_sortnet.h),
// then a window of `keep` sorted positions slides up from position 0 while the value it would gain at the top
// lies closer to the upper median than the value it would lose at the bottom lies to the lower median
// (d_hi < d_lo in fp32, false on NaN), and the window is added ascending from +0 and divided by keep.  keep is
// wave-uniform; the window's start j is not: it depends on the lane's data.
//
// The three forms of fa_trimmed.hip, with the same loads, stores and grids.  What is new is the access to
// s[j + keep] and the sum over [j, j + keep):
//   vector and element form (P = 2 .. 64, keys in registers): a second register array holds the keys shifted
//     down by keep, up[u] = s[u + keep], made by log2(P) conditional shifts by 1, 2, 4 ... under the bits of
//     keep -- wave-uniform branches around compile-time moves, never a runtime register index (that would go to
//     scratch).  The slide is a compile-time loop over u with a per-lane "still sliding" flag, the sum a
//     compile-time loop with the per-lane guard j <= u < j + keep.  P more registers, no LDS: the lane's own
//     LDS column would take P * 256 * 4 bytes per workgroup (64 KiB at P = 64) and cap the waves per CU below
//     what the registers allow.
//   wide form (64 < nc <= 128): the two sorted halves already live in the lane's LDS column, and the slide needs
//     the merged sequence at two runtime positions, so the merge writes it back into the same column.  The
//     column has 192 rows: half 0 in rows 64 .. 127, half 1 in rows 128 .. 191, the merged run from row 0.
//     Merged position p = a + b is written while the heads are read at rows 64 + a and 128 + b; both are above
//     p as long as b < 64 and a < 64, and a head whose half is exhausted is not read any more (it is the pad),
//     so a write never reaches a key that is still to be read.  The keys at the two heads are in registers
//     before the write.  48 KiB of LDS per one-wave workgroup: 3 workgroups per CU (the trimmed wide form:
//     32 KiB, 5).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"
#include "fa_sortnet.h"

namespace fa {

namespace {

// Rule 4 from the sorted keys s (nc live, pads above): the slide, the sum, the division.
template <int P>
__device__ __forceinline__ float centered_mean(const uint32_t (&s)[P], int nc, int keep, float div) {
    // up[u] = s[u + keep]: conditional shifts by the bits of keep (keep == P has none below log2 P and no slide)
    uint32_t up[P];
#pragma unroll
    for (int u = 0; u < P; ++u) up[u] = s[u];
#pragma unroll
    for (int sh = 1; sh < P; sh <<= 1) {
        if (keep & sh) {
#pragma unroll
            for (int u = 0; u < P; ++u) up[u] = u + sh < P ? up[u + sh] : 0xffffffffu;
        }
    }
    const int m_lo = (nc - 1) / 2, m_hi = nc / 2, slides = nc - keep;
    float c_lo = 0.0f, c_hi = 0.0f;
#pragma unroll
    for (int u = 0; u < P; ++u) {
        if (u == m_lo) c_lo = trim_value(s[u]);
        if (u == m_hi) c_hi = trim_value(s[u]);
    }
    int j = 0;
    bool sliding = true;
#pragma unroll
    for (int u = 0; u < P - 1; ++u) {  // slides <= P - 1
        if (u < slides) {
            const float d_hi = trim_value(up[u]) - c_hi;
            const float d_lo = c_lo - trim_value(s[u]);
            sliding = sliding && d_hi < d_lo;
            j += sliding ? 1 : 0;
        }
    }
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < P; ++u)
        if (u >= j && u < j + keep) acc = acc + trim_value(s[u]);
    return acc / div;
}

// Vector form: lane-vector v covers elements head + v*V .. + V-1 of every bucket (16-byte aligned there).
template <typename IN, typename OUT, int P, int SP>
__global__ __launch_bounds__(256) void centered_vec_kernel(const ClientTable t, int nc, int keep, float div, void* out,
                                                           int64_t head, int64_t nvec) {
    constexpr int V = In<IN>::kVec;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
        const int64_t e = head + v * V;
        u32x4 raw[P];  // every client's load in flight before the first key
#pragma unroll
        for (int u = 0; u < P; ++u)
            if (client_live<P>(u, nc)) raw[u] = ld16<true>(reinterpret_cast<const IN*>(t.src[u]) + e);
        uint32_t key[V][P];
#pragma unroll
        for (int u = 0; u < P; ++u) {
            if (client_live<P>(u, nc)) {
                float x[V];
                In<IN>::widen(raw[u], x);
#pragma unroll
                for (int j = 0; j < V; ++j) key[j][u] = trim_key(x[j]);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) key[j][u] = 0xffffffffu;
            }
        }
        float r[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sort_keys<P>(key[j]);
            r[j] = centered_mean<P>(key[j], nc, keep, div);
        }
        Out<OUT>::template store<V, SP>(out, e, r);
    }
}

// Element form over elements [0, head) and [tail0, n) (the whole bucket: head = tail0 = n), one per lane.
template <typename IN, typename OUT, int P>
__global__ __launch_bounds__(256) void centered_elem_kernel(const ClientTable t, int nc, int keep, float div, void* out,
                                                            int64_t head, int64_t tail0, int64_t n) {
    const int64_t cnt = head + (n - tail0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cnt; s += stride) {
        const int64_t i = s < head ? s : tail0 + (s - head);
        float x[P];
#pragma unroll
        for (int u = 0; u < P; ++u)
            if (client_live<P>(u, nc)) x[u] = In<IN>::scalar(t.src[u], i);
        uint32_t key[P];
#pragma unroll
        for (int u = 0; u < P; ++u) key[u] = client_live<P>(u, nc) ? trim_key(x[u]) : 0xffffffffu;
        sort_keys<P>(key);
        Out<OUT>::scalar(out, i, centered_mean<P>(key, nc, keep, div));
    }
}

// Wide form, 64 < nc <= 128, one element per lane, one wave per block (the file comment): no lane reads
// another's column, so no barrier.  The merge takes the lower head (ties: either, equal keys are
// interchangeable); an exhausted half reads as the pad 0xFFFFFFFF, taken only when every key left is a NaN key.
constexpr int kWideRows = 192;
template <typename IN, typename OUT>
__global__ __launch_bounds__(kWideBlock) void centered_wide_kernel(const ClientTable t, int nc, int keep, float div,
                                                                   void* out, int64_t n) {
    __shared__ uint32_t tile[kWideRows][kWideBlock];
    const int lane = threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kWideBlock;
    for (int64_t i = (int64_t)blockIdx.x * kWideBlock + lane; i < n; i += stride) {
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int base = 64 * h;
            float x[64];
#pragma unroll
            for (int u = 0; u < 64; ++u)
                if (base + u < nc) x[u] = In<IN>::scalar(t.src[base + u], i);
            uint32_t key[64];
#pragma unroll
            for (int u = 0; u < 64; ++u) key[u] = base + u < nc ? trim_key(x[u]) : 0xffffffffu;
            sort_keys<64>(key);
#pragma unroll
            for (int u = 0; u < 64; ++u) tile[64 + base + u][lane] = key[u];
        }
        int a = 0, b = 0;
        uint32_t ka = tile[64][lane], kb = tile[128][lane];
#pragma unroll 1
        for (int p = 0; p < nc; ++p) {  // p = a + b < 128
            const bool ta = ka <= kb;
            tile[p][lane] = ta ? ka : kb;
            a += ta ? 1 : 0;
            b += ta ? 0 : 1;
            const int q = ta ? a : b;
            const uint32_t next = q < 64 ? tile[(ta ? 64 : 128) + q][lane] : 0xffffffffu;
            ka = ta ? next : ka;
            kb = ta ? kb : next;
        }
        const float c_lo = trim_value(tile[(nc - 1) / 2][lane]), c_hi = trim_value(tile[nc / 2][lane]);
        int j = 0;
#pragma unroll 1
        while (j < nc - keep) {  // rows j and j + keep < nc
            const float d_hi = trim_value(tile[j + keep][lane]) - c_hi;
            const float d_lo = c_lo - trim_value(tile[j][lane]);
            if (!(d_hi < d_lo)) break;
            ++j;
        }
        float acc = 0.0f;
#pragma unroll 1
        for (int u = j; u < j + keep; ++u) acc = acc + trim_value(tile[u][lane]);  // j + keep <= nc
        Out<OUT>::scalar(out, i, acc / div);
    }
}

template <typename IN, typename OUT, int P>
hipError_t launch_centered_p(const ClientTable& t, int nc, int keep, void* out, const Split& sp, const Tuning& tu,
                             hipStream_t s) {
    constexpr int V = In<IN>::kVec;
    const float div = (float)keep;
    if constexpr (P * V <= 128) {
        if (sp.vec && sp.nvec > 0) {
            // nt loads, write-through stores: every byte is touched once (as the trimmed kernels)
            hipLaunchKernelGGL((centered_vec_kernel<IN, OUT, P, kStSc1>),
                               dim3((unsigned)blocks_for(sp.nvec, tu, (int64_t)1 << 30)), dim3(tu.block), 0, s, t,
                               nc, keep, div, out, sp.head, sp.nvec);
            if (sp.edges() > 0)
                hipLaunchKernelGGL((centered_elem_kernel<IN, OUT, P>), dim3(1), dim3(64), 0, s, t, nc, keep, div, out,
                                   sp.head, sp.tail0(), sp.n);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((centered_elem_kernel<IN, OUT, P>), dim3((unsigned)blocks_for(sp.n, tu, kElemMaxBlocks)),
                       dim3(tu.block), 0, s, t, nc, keep, div, out, sp.n, sp.n, sp.n);
    return hipGetLastError();
}

template <typename IN, typename OUT>
hipError_t launch_centered_t(const ClientTable& t, int nc, int keep, void* out, const Split& sp, const Tuning& tu,
                             hipStream_t s) {
#define FA_CENTER_P(P) \
    if (nc <= P) return launch_centered_p<IN, OUT, P>(t, nc, keep, out, sp, tu, s)
    FA_CENTER_P(2);
    FA_CENTER_P(4);
    FA_CENTER_P(8);
    FA_CENTER_P(16);
    FA_CENTER_P(32);
    FA_CENTER_P(64);
#undef FA_CENTER_P
    int64_t g = std::min<int64_t>((sp.n + kWideBlock - 1) / kWideBlock, kElemMaxBlocks);
    if (tu.max_blocks > 0) g = std::min<int64_t>(g, tu.max_blocks);
    hipLaunchKernelGGL((centered_wide_kernel<IN, OUT>), dim3((unsigned)std::max<int64_t>(1, g)), dim3(kWideBlock), 0, s,
                       t, nc, keep, (float)keep, out, sp.n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_centered(const ClientTable& t, int nc, fa_dtype in, fa_dtype out, int keep, void* dst,
                           const Split& sp, const Tuning& tu, hipStream_t s) {
    if (!sp.valid() || sp.V != (in == FA_F32 ? 4 : 8)) return hipErrorInvalidValue;
    if (nc < 1 || nc > FA_TRIMMED_MAX_CLIENTS || keep < 1 || keep > nc || !dtype_pair_ok(in, out))
        return hipErrorInvalidValue;
    auto with_out = [&](auto i) {
        using IN = decltype(i);
        if (out == FA_F32) return launch_centered_t<IN, float>(t, nc, keep, dst, sp, tu, s);
        if constexpr (sizeof(IN) == 2) {  // a 16-bit input keeps its own type or widens to fp32
            return launch_centered_t<IN, IN>(t, nc, keep, dst, sp, tu, s);
        } else {
            if (out == FA_BF16)
                return launch_centered_t<IN, uint16_t>(t, nc, keep, dst, sp, tu, s);
            return launch_centered_t<IN, _Float16>(t, nc, keep, dst, sp, tu, s);
        }
    };
    switch (in) {
        case FA_F32: return with_out(float{});
        case FA_BF16: return with_out(uint16_t{});
        case FA_F16: return with_out(_Float16{});
    }
    return hipErrorInvalidValue;
}

}  // namespace fa
