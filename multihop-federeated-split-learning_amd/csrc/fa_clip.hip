// fa_clip.hip -- the clip stage's norm pass (fa.h "Clip stage") for CDNA4 (gfx950): for every client k of a
// pass, Q_k = sum_i ((double)fl32(x_{k,i} - g_i))^2 over the n elements of a bucket, g the fp32 reference.
//
// It is the library's only reduction across elements.  A workgroup of 256 lanes owns tiles of 4096 elements:
// it loads the tile of g once into registers (16 floats per lane, 16-byte loads), then walks the clients of
// the pass with 16-byte non-temporal loads (the next client's loads are issued before this one's arithmetic),
// accumulates d * d per lane in fp64, adds the 64 lanes of each wave with an xor butterfly and keeps one fp64
// sum per (wave, client) in LDS while it strides over its tiles.  At the end it adds the four waves' sums in
// wave order and writes one partial per (client, workgroup).  A second launch, one wave per client, adds a
// client's partials: lane l takes partials l, l + 64, ... in ascending order, then the same butterfly.  There
// is no atomic anywhere, so for one layout (n, grid, pointer phases) every run gives the same bits; the order
// itself is not part of the rule (fa.h bounds the error of any order).
//
// Numerics (sq_add of fa_device.h, shared with fa_krum.hip): d = x - g is one fp32 subtraction of the exactly
// widened input; (double)d * (double)d is exact in fp64 (24 x 24 significand bits), so fma(dd, dd, acc) is the
// single rounding of the add.  Contraction is off for the TU all the same, as in fa_server_opt.hip: nothing
// here may change by the compiler's choice.  The grid is measure_grid of fa_split.h over tiles of 4096 elements.
//
// Two forms, as the other kernel TUs: the vector form when every client and the reference share one 16-byte
// phase, and the element form (one element per lane and load) for the head, the tail and mixed phases.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kClipThreads = kMeasureThreads;
constexpr int kClipLaneElems = 16;                                  // elements of g a lane keeps in registers
constexpr int64_t kClipTile = (int64_t)kClipThreads * kClipLaneElems;  // elements per tile

// LDS: one fp64 sum per (wave, client) (MeasureLds, lds_zero and lds_flush of fa_device.h).
using ClipLds = MeasureLds<kMaxClients>;

// Vector form: vector v of a bucket is elements head + V v .. + V - 1 (16-byte aligned in every client, and in
// ref for its 4-element vectors).  Tile `tile` is vectors [tile * 256 R, + 256 R), lane-interleaved.
template <typename T>
__global__ __launch_bounds__(kClipThreads) void clip_sumsq_vec_kernel(const ClientTable t, int nc, const float* ref,
                                                                       int64_t head, int64_t nvec, double* partials,
                                                                       int64_t pstride) {
    constexpr int V = In<T>::kVec, R = kClipLaneElems / V;
    __shared__ ClipLds lds;
    lds_zero(lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile_vecs = (int64_t)kClipThreads * R;
    const int64_t ntiles = (nvec + tile_vecs - 1) / tile_vecs;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int64_t e[R];    // the first element of the lane's r-th vector
        bool live[R];
        float g[kClipLaneElems];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t v = tile * tile_vecs + (int64_t)r * kClipThreads + threadIdx.x;
            live[r] = v < nvec;
            e[r] = head + (live[r] ? v : 0) * V;
#pragma unroll
            for (int q = 0; q < V / 4; ++q) {
                u32x4 rg = {};
                if (live[r]) rg = ld16<false>(ref + e[r] + 4 * q);
                In<float>::widen(rg, g + r * V + 4 * q);
            }
        }
        u32x4 cur[R], nxt[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            cur[r] = u32x4{};
            nxt[r] = u32x4{};
            if (live[r]) cur[r] = ld16<true>(reinterpret_cast<const T*>(t.src[0]) + e[r]);
        }
        for (int k = 0; k < nc; ++k) {
            if (k + 1 < nc) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (live[r]) nxt[r] = ld16<true>(reinterpret_cast<const T*>(t.src[k + 1]) + e[r]);
            }
            double a = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float x[V];
                In<T>::widen(cur[r], x);
                if (live[r]) {
#pragma unroll
                    for (int j = 0; j < V; ++j) a = sq_add(x[j], g[r * V + j], a);
                }
            }
            a = wave_sum(a);
            if (lane == 0) lds.acc[wave][k] += a;
#pragma unroll
            for (int r = 0; r < R; ++r) cur[r] = nxt[r];
        }
    }
    lds_flush(lds, nc, partials, pstride, blockIdx.x);
}

// Element form over elements [0, head) and [tail0, n) (the whole array: head = tail0 = n), one element per lane
// and load; its partials go to slots slot0 + blockIdx.x.
template <typename T>
__global__ __launch_bounds__(kClipThreads) void clip_sumsq_elem_kernel(const ClientTable t, int nc, const float* ref,
                                                                        int64_t head, int64_t tail0, int64_t n,
                                                                        double* partials, int64_t pstride, int64_t slot0) {
    __shared__ ClipLds lds;
    lds_zero(lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cnt = head + (n - tail0);
    const int64_t ntiles = (cnt + kClipTile - 1) / kClipTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int64_t idx[kClipLaneElems];
        bool live[kClipLaneElems];
        float g[kClipLaneElems];
#pragma unroll
        for (int r = 0; r < kClipLaneElems; ++r) {
            const int64_t s = tile * kClipTile + (int64_t)r * kClipThreads + threadIdx.x;
            live[r] = s < cnt;
            idx[r] = !live[r] ? 0 : s < head ? s : tail0 + (s - head);
            g[r] = live[r] ? ref[idx[r]] : 0.0f;
        }
        for (int k = 0; k < nc; ++k) {
            const void* src = t.src[k];
            double a = 0.0;
#pragma unroll
            for (int r = 0; r < kClipLaneElems; ++r)
                if (live[r]) a = sq_add(In<T>::scalar(src, idx[r]), g[r], a);
            a = wave_sum(a);
            if (lane == 0) lds.acc[wave][k] += a;
        }
    }
    lds_flush(lds, nc, partials, pstride, slot0 + blockIdx.x);
}

// One wave per client: sums[k] = the client's np partials, lane l adding l, l + 64, ... in ascending order.
__global__ __launch_bounds__(64) void clip_finish_kernel(const double* partials, int64_t pstride, int64_t np,
                                                         double* sums) {
    const double* p = partials + (int64_t)blockIdx.x * pstride;
    double a = 0.0;
    for (int64_t b = threadIdx.x; b < np; b += 64) a += p[b];
    a = wave_sum(a);
    if (threadIdx.x == 0) sums[blockIdx.x] = a;
}

// dst[i] = (float)src[i], exact (bf16, fp16 with its subnormals, signed zeros kept).
template <typename T>
__global__ __launch_bounds__(256) void clip_widen_kernel(const void* src, float* dst, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = In<T>::scalar(src, i);
}

template <typename T>
hipError_t launch_sumsq_t(const ClientTable& t, int nc, const float* ref, const Split& sp, const MeasureGrid& gr,
                          double* partials, double* sums, hipStream_t s) {
    const int64_t np = gr.np();
    if (gr.vec_blocks > 0) {
        hipLaunchKernelGGL((clip_sumsq_vec_kernel<T>), dim3((unsigned)gr.vec_blocks), dim3(kClipThreads), 0, s, t, nc, ref,
                           sp.head, sp.nvec, partials, np);
        if (gr.elem_blocks > 0)
            hipLaunchKernelGGL((clip_sumsq_elem_kernel<T>), dim3(1), dim3(kClipThreads), 0, s, t, nc, ref, sp.head,
                               sp.tail0(), sp.n, partials, np, gr.vec_blocks);
    } else {
        hipLaunchKernelGGL((clip_sumsq_elem_kernel<T>), dim3((unsigned)gr.elem_blocks), dim3(kClipThreads), 0, s, t, nc,
                           ref, sp.n, sp.n, sp.n, partials, np, (int64_t)0);
    }
    return launch_measure_finish(partials, np, nc, sums, s);
}

}  // namespace

hipError_t launch_measure_finish(const double* partials, int64_t np, int rows, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(clip_finish_kernel, dim3((unsigned)rows), dim3(64), 0, s, partials, np, np, sums);
    return hipGetLastError();
}

hipError_t launch_clip_sumsq(const ClientTable& t, int nc, fa_dtype in, const float* ref, const Split& sp,
                             double* partials, double* sums, const Tuning& tu, hipStream_t s) {
    if (!sp.valid() || sp.V != (in == FA_F32 ? 4 : 8)) return hipErrorInvalidValue;
    if (nc < 1 || nc > kMaxClients || sp.n <= 0 || !ref || !partials || !sums) return hipErrorInvalidValue;
    const MeasureGrid gr = measure_grid(sp, kClipTile, kClipMaxBlocks, tu.max_blocks);
    switch (in) {
        case FA_F32: return launch_sumsq_t<float>(t, nc, ref, sp, gr, partials, sums, s);
        case FA_BF16: return launch_sumsq_t<uint16_t>(t, nc, ref, sp, gr, partials, sums, s);
        case FA_F16: return launch_sumsq_t<_Float16>(t, nc, ref, sp, gr, partials, sums, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_clip_widen(const void* src, fa_dtype dt, float* dst, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!src || !dst) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1 << 16));
    switch (dt) {
        case FA_F32: hipLaunchKernelGGL((clip_widen_kernel<float>), dim3(grid), dim3(256), 0, s, src, dst, n); break;
        case FA_BF16: hipLaunchKernelGGL((clip_widen_kernel<uint16_t>), dim3(grid), dim3(256), 0, s, src, dst, n); break;
        case FA_F16: hipLaunchKernelGGL((clip_widen_kernel<_Float16>), dim3(grid), dim3(256), 0, s, src, dst, n); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fa
