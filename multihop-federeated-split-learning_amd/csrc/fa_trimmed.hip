// fa_trimmed.hip -- coordinate-wise trimmed mean / median (FA_TRIMMED) for CDNA4 (gfx950).
//
// Per element: the D client values, widened exactly to fp32, are mapped to unsigned keys whose integer order
// is the total order of fa.h (NaN above +inf, -0 below +0), sorted ascending, and the values at sorted
// positions [trim, D - trim) are added in that order from +0 and divided by D - 2 trim (fa.h "FA_TRIMMED").
//
// The sort is a network of integer compare-exchanges (v_min_u32 / v_max_u32: no NaN or canonicalisation
// rules of the float min/max) on keys that stay in registers: the kernels are templated on the padded width
// P = 2 .. 64, the network is fully unrolled, every index is a compile-time constant.  Clients D .. P-1 are
// padded with key 0xFFFFFFFF, which sorts last, so the window [trim, D - trim) never reaches a pad.  The
// window bounds are runtime values (wave-uniform): a compile-time loop over the P positions with a guarded
// add, never an index.
//
// P = 128 (D = 65 .. 128) is the wide form: the unrolled 1792-exchange network did not compile in bounded
// time, and it is not the cheapest way either.  The two halves of 64 clients are each sorted in registers by
// the 64-wide network (2 x 672 exchanges), written to the lane's own column of an LDS tile, and merged by a
// two-pointer walk over the D - trim lowest positions, which adds the window as it goes.  The walk needs
// runtime indices, which is why the sorted halves live in LDS and not in registers (DESIGN.md "Trimmed mean").
//
// Two forms.  The vector form (P * V <= 128 keys per lane: f32 up to P = 32, bf16 / fp16 up to P = 16) loads
// 16 bytes per client per lane as the FedAvg chain does and sorts its V elements side by side.  The element
// form holds one element per lane (P keys): it is the main body for the wider P, where the sort and not the
// load width bounds the kernel, and everywhere the path for the head, the tail and inputs of mixed 16-byte
// phase.  Register use per P: DESIGN.md "Trimmed mean".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"
#include "fa_sortnet.h"

namespace fa {

namespace {

// fl(sum of the kept positions, ascending, from +0) / div.
template <int P>
__device__ __forceinline__ float window_mean(const uint32_t (&k)[P], int lo, int hi, float div) {
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < P; ++u)
        if (u >= lo && u < hi) acc = acc + trim_value(k[u]);
    return acc / div;
}

// Vector form: lane-vector v covers elements head + v*V .. + V-1 of every bucket (16-byte aligned there).
template <typename IN, typename OUT, int P, int SP>
__global__ __launch_bounds__(256) void trimmed_vec_kernel(const ClientTable t, int nc, int trim, float div, void* out,
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
            r[j] = window_mean<P>(key[j], trim, nc - trim, div);
        }
        Out<OUT>::template store<V, SP>(out, e, r);
    }
}

// Element form over elements [0, head) and [tail0, n) (the whole bucket: head = tail0 = n), one per lane.
template <typename IN, typename OUT, int P>
__global__ __launch_bounds__(256) void trimmed_elem_kernel(const ClientTable t, int nc, int trim, float div, void* out,
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
        Out<OUT>::scalar(out, i, window_mean<P>(key, trim, nc - trim, div));
    }
}

// Wide form, 64 < nc <= 128, one element per lane, one wave per block: half h holds clients 64 h .. 64 h + 63,
// sorted in registers and kept in rows 64 h .. of the lane's LDS column (no lane reads another's column, so
// no barrier).  The merge takes the lower head (ties: either, equal keys are interchangeable), and a head
// past its half's end reads as the pad 0xFFFFFFFF: it is taken only when the other head is a pad or NaN key
// too, and then every key left decodes to the same NaN.
template <typename IN, typename OUT>
__global__ __launch_bounds__(kWideBlock) void trimmed_wide_kernel(const ClientTable t, int nc, int trim, float div,
                                                                  void* out, int64_t n) {
    __shared__ uint32_t tile[128][kWideBlock];
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
            for (int u = 0; u < 64; ++u) tile[base + u][lane] = key[u];
        }
        const int hi = nc - trim;
        int a = 0, b = 0;
        uint32_t ka = tile[0][lane], kb = tile[64][lane];
        float acc = 0.0f;
#pragma unroll 1
        for (int p = 0; p < hi; ++p) {
            const bool ta = ka <= kb;
            if (p >= trim) acc = acc + trim_value(ta ? ka : kb);
            a += ta ? 1 : 0;
            b += ta ? 0 : 1;
            const int q = ta ? a : b;
            const uint32_t next = q < 64 ? tile[(ta ? 0 : 64) + q][lane] : 0xffffffffu;
            ka = ta ? next : ka;
            kb = ta ? kb : next;
        }
        Out<OUT>::scalar(out, i, acc / div);
    }
}

template <typename IN, typename OUT, int P>
hipError_t launch_trimmed_p(const ClientTable& t, int nc, int trim, void* out, const Split& sp, const Tuning& tu,
                            hipStream_t s) {
    constexpr int V = In<IN>::kVec;
    const float div = (float)(nc - 2 * trim);
    if constexpr (P * V <= 128) {
        if (sp.vec && sp.nvec > 0) {
            // nt loads, write-through stores: every byte is touched once (as the literal kernel)
            hipLaunchKernelGGL((trimmed_vec_kernel<IN, OUT, P, kStSc1>),
                               dim3((unsigned)blocks_for(sp.nvec, tu, (int64_t)1 << 30)), dim3(tu.block), 0, s, t,
                               nc, trim, div, out, sp.head, sp.nvec);
            if (sp.edges() > 0)
                hipLaunchKernelGGL((trimmed_elem_kernel<IN, OUT, P>), dim3(1), dim3(64), 0, s, t, nc, trim, div, out,
                                   sp.head, sp.tail0(), sp.n);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((trimmed_elem_kernel<IN, OUT, P>), dim3((unsigned)blocks_for(sp.n, tu, kElemMaxBlocks)),
                       dim3(tu.block), 0, s, t, nc, trim, div, out, sp.n, sp.n, sp.n);
    return hipGetLastError();
}

template <typename IN, typename OUT>
hipError_t launch_trimmed_t(const ClientTable& t, int nc, int trim, void* out, const Split& sp, const Tuning& tu,
                            hipStream_t s) {
#define FA_TRIM_P(P) \
    if (nc <= P) return launch_trimmed_p<IN, OUT, P>(t, nc, trim, out, sp, tu, s)
    FA_TRIM_P(2);
    FA_TRIM_P(4);
    FA_TRIM_P(8);
    FA_TRIM_P(16);
    FA_TRIM_P(32);
    FA_TRIM_P(64);
#undef FA_TRIM_P
    int64_t g = std::min<int64_t>((sp.n + kWideBlock - 1) / kWideBlock, kElemMaxBlocks);
    if (tu.max_blocks > 0) g = std::min<int64_t>(g, tu.max_blocks);
    hipLaunchKernelGGL((trimmed_wide_kernel<IN, OUT>), dim3((unsigned)std::max<int64_t>(1, g)), dim3(kWideBlock), 0, s,
                       t, nc, trim, (float)(nc - 2 * trim), out, sp.n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_trimmed(const ClientTable& t, int nc, fa_dtype in, fa_dtype out, int trim, void* dst,
                          const Split& sp, const Tuning& tu, hipStream_t s) {
    if (!sp.valid() || sp.V != (in == FA_F32 ? 4 : 8)) return hipErrorInvalidValue;
    if (nc < 1 || nc > FA_TRIMMED_MAX_CLIENTS || trim < 0 || 2 * trim >= nc || !dtype_pair_ok(in, out))
        return hipErrorInvalidValue;
    auto with_out = [&](auto i) {
        using IN = decltype(i);
        if (out == FA_F32) return launch_trimmed_t<IN, float>(t, nc, trim, dst, sp, tu, s);
        if constexpr (sizeof(IN) == 2) {  // a 16-bit input keeps its own type or widens to fp32
            return launch_trimmed_t<IN, IN>(t, nc, trim, dst, sp, tu, s);
        } else {
            if (out == FA_BF16)
                return launch_trimmed_t<IN, uint16_t>(t, nc, trim, dst, sp, tu, s);
            return launch_trimmed_t<IN, _Float16>(t, nc, trim, dst, sp, tu, s);
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
