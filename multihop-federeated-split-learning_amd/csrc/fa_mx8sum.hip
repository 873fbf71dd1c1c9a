// fa_mx8sum.hip -- the MX8-sum stage (fa.h "MX8-sum stage") for CDNA4 (gfx950): the MX8 receipts of a round reduced
// straight from their code streams into the fp32 aggregate, a_i = g_i + sum_c w_c d_c,i, without expanding a receipt
// into a dense slot.  Per element the kernel reads one byte of q per client, one scale byte per client and 32
// elements, g once, and writes the output once: 1.03 D + 8 bytes with f32 g and output, where fa_submit_mx8 and the
// chain move about 13 D + 4.
//
// Vector form.  A lane owns 16 consecutive elements: one 16-byte load of q per client, half a block of 32.  A wave owns
// 1024 elements, a workgroup of 256 lanes a tile of 4096 elements, and tiles are dealt over a grid of what is
// co-resident, the rest strided.  Tiles are laid on the blocks of the bucket, not on the launch: tile 0 starts at the
// block boundary at or before the first vector element (`pad` = 0 or 16 elements early; the lanes before the first
// vector and after the last sit idle), so every tile covers exactly 128 blocks and a lane's block is lane >> 1.
//   Scales through LDS: per tile the workgroup copies the D x 128 scale bytes, row c = client c, into 16 KiB of LDS.
//   A wave takes every fourth row, its 64 lanes two bytes each: one 2-byte load where the address is even (a
//   context's always is: shadows start on 256 bytes and pieces on multiples of 64 elements, two blocks), else two
//   byte loads; the bytes beyond the launch's blocks are not read and count as 0.  The row is wave-uniform, so the
//   table is read by scalar loads here too.  A barrier, then each lane takes its one byte per client from LDS (two lanes share
//   it; the 64 lanes of a wave read 32 consecutive bytes, a broadcast per dword) and builds the fp32 scale from it by
//   integer operations (mx8_scale_bits: a subnormal pattern below E = 7, a quiet NaN at 255).  No lane issues a global
//   byte load per client.  A second barrier before the next tile's copy.
//   Registers: 16 fp32 accumulators; the q words of the next kMx8SumGroup = 4 clients are in flight (non-temporal
//   16-byte loads) under the 16 multiplies and 16 fused multiply-adds of each current one; bytes are sign-extended by a
//   shift pair and converted in registers.  Then g in 16-byte loads, one add, 16-byte stores.
// Element form: one element per lane, client by client, every byte of q and e by its own load: correct at any byte
// phase of q and e, any element phase of g and the output and any idx0.  It takes the few elements before the first
// and after the last vector (one workgroup of 64) and whole launches whose operands do not allow the vector form
// (mx8sum_split).  Both forms do the same three operations per client and element, so the bits do not depend on it.
//
// The client table -- q, e and w of up to 128 clients, 2.5 KiB -- travels in the kernel-argument segment (4 KiB), as
// fa_sparse.hip's does: no upload, and every access to it is a scalar load with a wave-uniform index.
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950): the vector kernels take 62 - 64 VGPRs in every dtype
// pair, 0 AGPRs, 16384 bytes of LDS, no scratch, no spills, 8 waves per SIMD -- 8 workgroups per CU, which is the grid's
// cap; the element kernels 14 - 15 VGPRs, no LDS, no scratch.  Measured: 0.105 - 0.176 of the expanded
// route's device time at D = 64 .. 8, at 4.7 TB/s of its own byte model.
//
// Bit-exactness: `#pragma clang fp contract(off)`.  The fp32 operations are the multiply of rule 1, the fused
// multiply-add of rule 2 (written as one) and the add of rule 3; the scale is never folded into the weight.  The file is
// compiled without packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "fa_device.h"
#include "fa_host.h"
#include "fa_internal.h"
#include "fa_mx8.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kLane = 16;                    // the elements of a lane: one 16-byte load of q
constexpr int kThreads = 256;
constexpr int kTile = kMx8SumTile;           // the elements of a workgroup's tile
constexpr int kBlocks = kTile / 32;          // its blocks: the scale bytes per client in LDS
constexpr int kGroup = kMx8SumGroup;         // the clients whose q words are in flight
constexpr int64_t kMaxGrid = 256 * 8;        // 256 CUs x the workgroups co-resident on one; tiles beyond it are strided
static_assert(kTile == kThreads * kLane && kBlocks == 128, "a lane owns 16 elements, a tile 128 blocks");

struct NoRef {};

struct Mx8SumTable {  // 2.5 KiB of the kernel-argument segment
    const int8_t* q[kMaxClients];
    const uint8_t* e[kMaxClients];
    float w[kMaxClients];
};

// One launch: n elements, bucket elements idx0 ..; the vector form takes [head, tail0), laid `pad` elements into the
// first of `tiles` tiles; nscale: the scale bytes of the launch's blocks.
struct Mx8SumLanes {
    int64_t n, head, tail0, tiles, nscale;
    uint64_t idx0;
    int pad, D;
};

__device__ __forceinline__ float sum_fma(float w, float d, float acc) { return __builtin_fmaf(w, d, acc); }

// Rules 1-2 for one client on a lane's 16 elements: the codes in wq, the scale s, the weight w.
__device__ __forceinline__ void apply16(const u32x4 wq, float s, float w, float* acc) {
#pragma unroll
    for (int k = 0; k < kLane; ++k) {
        const int qk = (int)(wq[k >> 2] << (24 - 8 * (k & 3))) >> 24;  // byte k & 3, sign-extended
        acc[k] = sum_fma(w, mx8_delta(qk, s), acc[k]);
    }
}

template <typename DST, typename REF>
__global__ __launch_bounds__(kThreads) void mx8sum_vec_kernel(const Mx8SumTable tb, const Mx8SumLanes ln, const void* ref,
                                                              void* dst) {
    __shared__ __attribute__((aligned(16))) uint8_t sc[kMaxClients * kBlocks];
    const int tid = (int)threadIdx.x, D = ln.D;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t base = ln.head - ln.pad;  // the element of tile 0's first lane: on a block boundary of the bucket
    const int64_t eb00 = (int64_t)(((ln.idx0 + (uint64_t)ln.head - (uint64_t)ln.pad) >> 5) - (ln.idx0 >> 5));
    for (int64_t t = blockIdx.x; t < ln.tiles; t += gridDim.x) {
        // the tile's scales: row c = the bytes eb0 .. eb0 + 127 of client c, those beyond the launch's blocks as 0
        const int64_t eb0 = eb00 + t * kBlocks;
        for (int c = wave; c < D; c += kThreads / 64) {  // wave-uniform: the table is read by scalar loads
            const int j = 2 * (tid & 63);
            const uint8_t* p = tb.e[c] + eb0 + j;
            uint32_t v = 0;
            if (eb0 + j + 2 <= ln.nscale && ((uintptr_t)p & 1u) == 0) {
                v = *reinterpret_cast<const uint16_t*>(p);
            } else {
                if (eb0 + j < ln.nscale) v = p[0];
                if (eb0 + j + 1 < ln.nscale) v |= (uint32_t)p[1] << 8;
            }
            *reinterpret_cast<uint16_t*>(&sc[c * kBlocks + j]) = (uint16_t)v;
        }
        __syncthreads();
        const int64_t el = base + t * kTile + (int64_t)tid * kLane;
        if (el >= ln.head && el + kLane <= ln.tail0) {  // else a lane before the first or after the last vector
            const uint8_t* my = &sc[tid >> 1];
            const auto fetch = [&](int c0, u32x4* ch) {
#pragma unroll
                for (int u = 0; u < kGroup; ++u)
                    ch[u] = c0 + u < D ? ld16<true>(tb.q[c0 + u] + el) : u32x4{0u, 0u, 0u, 0u};
            };
            float acc[kLane];
#pragma unroll
            for (int k = 0; k < kLane; ++k) acc[k] = 0.0f;
            u32x4 cur[kGroup], nxt[kGroup];
            fetch(0, cur);
            for (int c0 = 0; c0 < D; c0 += kGroup) {
                fetch(c0 + kGroup, nxt);
#pragma unroll
                for (int u = 0; u < kGroup; ++u)
                    if (c0 + u < D) apply16(cur[u], mx8_scale(my[(c0 + u) * kBlocks]), tb.w[c0 + u], acc);
#pragma unroll
                for (int u = 0; u < kGroup; ++u) cur[u] = nxt[u];
            }
            if constexpr (!__is_same(REF, NoRef)) {
                float g[kLane];
                load_ref16<REF>(ref, el, g);
#pragma unroll
                for (int k = 0; k < kLane; ++k) acc[k] = mx8_add(g[k], acc[k]);
            }
            store16<DST>(dst, el, acc);
        }
        __syncthreads();  // the next tile overwrites the scales
    }
}

// Element form over elements [0, head) and [tail0, n) (the whole launch: head = tail0 = n), one per lane.
template <typename DST, typename REF>
__global__ __launch_bounds__(kThreads) void mx8sum_elem_kernel(const Mx8SumTable tb, const Mx8SumLanes ln, const void* ref,
                                                               void* dst) {
    const int64_t cnt = ln.head + (ln.n - ln.tail0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t b0 = ln.idx0 >> 5;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cnt; s += stride) {
        const int64_t i = s < ln.head ? s : ln.tail0 + (s - ln.head);
        const int64_t b = (int64_t)(((ln.idx0 + (uint64_t)i) >> 5) - b0);
        float acc = 0.0f;
        for (int c = 0; c < ln.D; ++c) acc = sum_fma(tb.w[c], mx8_delta((int)tb.q[c][i], mx8_scale(tb.e[c][b])), acc);
        if constexpr (!__is_same(REF, NoRef)) acc = mx8_add(In<REF>::scalar(ref, i), acc);
        Out<DST>::scalar(dst, i, acc);
    }
}

template <typename DST, typename REF>
void launch_t(const Mx8SumTable& tb, const Mx8SumLanes& ln, const void* ref, void* dst, int64_t cap, hipStream_t s) {
    const int64_t edges = ln.head + (ln.n - ln.tail0);
    if (ln.tiles > 0) {
        hipLaunchKernelGGL((mx8sum_vec_kernel<DST, REF>), dim3((unsigned)std::min(ln.tiles, cap)), dim3(kThreads), 0, s, tb,
                           ln, ref, dst);
        if (edges > 0) hipLaunchKernelGGL((mx8sum_elem_kernel<DST, REF>), dim3(1), dim3(64), 0, s, tb, ln, ref, dst);
        return;
    }
    const int64_t blocks = std::max<int64_t>(1, std::min((edges + kThreads - 1) / kThreads, cap));
    hipLaunchKernelGGL((mx8sum_elem_kernel<DST, REF>), dim3((unsigned)blocks), dim3(kThreads), 0, s, tb, ln, ref, dst);
}

template <typename DST>
void launch_d(const Mx8SumTable& tb, const Mx8SumLanes& ln, const void* ref, fa_dtype rdt, void* dst, int64_t cap,
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

// The split of one launch, led by the output (fa_split.h): the vector form needs the reference after the same head,
// every client's q on 16 bytes there, and the head's bucket index on a multiple of 16, so that a lane's 16 elements
// share a block.  Judged by the unclamped head: a launch that ends before it has no vector either way.
Split mx8sum_split(size_t n, const int8_t* const* q, int D, uint64_t idx0, const void* ref, fa_dtype rdt, const void* out,
                   fa_dtype odt) {
    Split sp = topk_split(out, odt == FA_F32 ? 4 : 2, n);
    sp.vec = (idx0 + (uint64_t)sp.lead) % kLane == 0;
    if (ref) sp.vec = sp.vec && sp.after(ref, sp.lead, rdt == FA_F32 ? 4 : 2);
    for (int c = 0; c < D; ++c) sp.vec = sp.vec && sp.after(q[c], sp.lead, 1);
    return sp;
}

hipError_t launch_mx8_sum(const int8_t* const* q, const uint8_t* const* e, const float* w, int D, uint64_t idx0, int64_t n,
                          const void* ref, fa_dtype rdt, void* out, fa_dtype odt, const Tuning& tu, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (D < 1 || D > kMaxClients || !q || !e || !w || !out || (ref && !dtype_pair_ok(rdt, odt))) return hipErrorInvalidValue;
    Mx8SumTable tb;
    for (int c = 0; c < kMaxClients; ++c) {
        const bool in = c < D;
        if (in && (!q[c] || !e[c])) return hipErrorInvalidValue;
        tb.q[c] = in ? q[c] : nullptr;
        tb.e[c] = in ? e[c] : nullptr;
        tb.w[c] = in ? w[c] : 0.0f;
    }
    const Split sp = mx8sum_split((size_t)n, q, D, idx0, ref, rdt, out, odt);
    if (!sp.valid()) return hipErrorInvalidValue;
    Mx8SumLanes ln{n, n, n, 0, (int64_t)(((idx0 + (uint64_t)n - 1) >> 5) - (idx0 >> 5)) + 1, idx0, 0, D};
    if (sp.vec && sp.nvec > 0) {
        ln.head = sp.head;
        ln.tail0 = sp.tail0();
        ln.pad = (int)((idx0 + (uint64_t)sp.head) & 31u);  // 0 or 16
        ln.tiles = (ln.pad + sp.nvec * kLane + kTile - 1) / kTile;
    }
    int64_t cap = kMaxGrid;
    if (tu.max_blocks > 0) cap = std::min<int64_t>(cap, tu.max_blocks);
    switch (odt) {
        case FA_F32: launch_d<float>(tb, ln, ref, rdt, out, cap, s); break;
        case FA_BF16: launch_d<uint16_t>(tb, ln, ref, rdt, out, cap, s); break;
        case FA_F16: launch_d<_Float16>(tb, ln, ref, rdt, out, cap, s); break;
    }
    return hipGetLastError();
}

// Rules 1-3 on the host: client by client, which is every element's chain in ascending client order.
void mx8_sum_host(const int8_t* const* q, const uint8_t* const* e, const float* w, int D, size_t n, uint64_t idx0,
                  const float* ref, float* out) {
#pragma clang fp contract(off)
    const uint64_t b0 = idx0 >> 5;
    std::fill(out, out + n, 0.0f);
    for (int c = 0; c < D; ++c)
        for (size_t i = 0; i < n; ++i)
            out[i] = std::fmaf(w[c], mx8_delta((int)q[c][i], mx8_scale(e[c][((idx0 + i) >> 5) - b0])), out[i]);
    for (size_t i = 0; ref && i < n; ++i) out[i] = ref[i] + out[i];
}

}  // namespace fa

using namespace fah;

namespace {

// What fa_mx8_sum_host, fa_mx8_sum_device and fa_mx8_sum_form refuse before they look at a pointer's target.
int check_mx8_sum(const void* const* q, const void* const* e, const float* w, int D, size_t n, uint64_t idx0) {
    if (D < 1 || D > FA_MX8_SUM_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "mx8 sum: D = %d clients outside 1 .. %d", D, FA_MX8_SUM_MAX_CLIENTS);
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "mx8 sum: idx0 + n beyond 2^64");
    if (n == 0) return FA_OK;
    if (!q || !e || !w) return fail(FA_ERR_ARG, "mx8 sum: %s is null", !q ? "q" : !e ? "e" : "w");
    for (int c = 0; c < D; ++c)
        if (!q[c] || !e[c]) return fail(FA_ERR_ARG, "mx8 sum: client %d's %s is null", c, !q[c] ? "q" : "e");
    return FA_OK;
}

// The operands of the dense side.
int check_mx8_sum_dense(size_t n, const void* d_ref, fa_dtype rdt, const void* d_out, fa_dtype odt) {
    if (!d_out) return fail(FA_ERR_ARG, "mx8 sum: d_out is null");
    if (d_ref && !aligned(d_ref, dsize(rdt))) return fail(FA_ERR_ALIGN, "mx8 sum: reference not %zu-byte aligned", dsize(rdt));
    if (!aligned(d_out, dsize(odt))) return fail(FA_ERR_ALIGN, "mx8 sum: output not %zu-byte aligned", dsize(odt));
    if (d_ref) {
        const uintptr_t o = (uintptr_t)d_out, r = (uintptr_t)d_ref;
        if (o < r + n * dsize(rdt) && r < o + n * dsize(odt)) return fail(FA_ERR_ARG, "mx8 sum: d_out overlaps d_ref");
    }
    return FA_OK;
}

}  // namespace

extern "C" {

int fa_mx8_sum_host(const int8_t* const* q, const uint8_t* const* e, const float* w, int D, size_t n, uint64_t idx0,
                    const float* ref, float* out) {
    g_err.clear();
    if (int rc = check_mx8_sum(reinterpret_cast<const void* const*>(q), reinterpret_cast<const void* const*>(e), w, D, n, idx0))
        return rc;
    if (n == 0) return FA_OK;
    if (!out) return fail(FA_ERR_ARG, "mx8 sum: out is null");
    fa::mx8_sum_host(q, e, w, D, n, idx0, ref, out);
    return FA_OK;
}

int fa_mx8_sum_device(fa_ctx* ctx, int gpu, const int8_t* const* d_q, const uint8_t* const* d_e, const float* w, int D, size_t n,
                      uint64_t idx0, const void* d_ref, fa_dtype ref_dtype, void* d_out, fa_dtype out_dtype, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!dvalid(out_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    FA_PAIR(ref_dtype, out_dtype);
    if (int rc = check_mx8_sum(reinterpret_cast<const void* const*>(d_q), reinterpret_cast<const void* const*>(d_e), w, D, n,
                               idx0))
        return rc;
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if (int rc = check_mx8_sum_dense(n, d_ref, ref_dtype, d_out, out_dtype)) return rc;
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_mx8_sum(d_q, d_e, w, D, idx0, (int64_t)n, d_ref, ref_dtype, d_out, out_dtype, c.tu, c.s));
    return FA_OK;
}

int fa_mx8_sum_form(size_t n, const int8_t* const* d_q, int D, uint64_t idx0, const void* d_ref, fa_dtype ref_dtype,
                    const void* d_out, fa_dtype out_dtype) {
    g_err.clear();
    if (!dvalid(out_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    FA_PAIR(ref_dtype, out_dtype);
    if (D < 1 || D > FA_MX8_SUM_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "mx8 sum: D = %d clients outside 1 .. %d", D, FA_MX8_SUM_MAX_CLIENTS);
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "mx8 sum: idx0 + n beyond 2^64");
    if (!d_q) return fail(FA_ERR_ARG, "mx8 sum: q is null");
    if (int rc = check_mx8_sum_dense(0, d_ref, ref_dtype, d_out, out_dtype)) return rc;
    return fa::mx8sum_split(n, d_q, D, idx0, d_ref, ref_dtype, d_out, out_dtype).vec ? FA_MX8_SUM_VECTOR : 0;
}

}  // extern "C"
