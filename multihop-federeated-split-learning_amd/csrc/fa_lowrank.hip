// fa_lowrank.hip -- low-rank receipts (fa.h "Low-rank receipts") for CDNA4 (gfx950): an update whose matrices arrive as
// factor pairs, M_j ~ P_j Q_j^T, expanded into an ordinary slot x = g + d.  The rank-r products go to the matrix unit:
// two widened fp32 values multiply exactly in fp64, and v_mfma_f64_16x16x4_f64 does 1024 such multiply-adds per issue
// (fa_gram.hip has the same trick for Y Y^T).
//
// Plan.  A host-only planner (lowrank_plan) walks the part's table once per launch range [idx0, idx0 + cnt): every
// matrix is cut into output tiles of 64 x 64 elements, of which those whose row band meets the range are listed, and
// the gaps between the matrices (`rest`) are cut into chunks of at most 2048 elements with their offsets in f.  The
// blob is a header and one 32-byte record per tile and per chunk; it does not depend on r (a record holds the rows and
// columns before its matrix, which r scales), so one plan serves owners of different ranks.  One launch, one workgroup
// of 256 lanes per record: block b takes tile b, the blocks after the tiles a rest chunk each.
//
// A tile.  The workgroup fills LDS with the tile's 64 rows of P and 64 rows of Q, each value converted to double once,
// the rank in chunks of at most 32 (a rank above 32 takes two fills into the same accumulators): rows are 34 doubles
// apart, dead rows and the rank's padding to a multiple of 4 are zeros.  Wave w owns the 16-row band w of the tile
// and its four 16 x 16 blocks: per k-step it reads one double of P and four of Q (the operand of lane l for a block is
// row l % 16, k = 4 s + l / 16 of its factor, A and B alike) and issues four MFMAs into 4 x 4 accumulator doubles per
// lane; bands and blocks that lie wholly past the matrix edge are skipped.  Row padding: within the lanes 0 .. 31 of
// a read (l % 16 = i, l / 16 = c in {0, 1}) the doubles lie 34 i + c apart, and 34 = 2 x 17 with 17 odd, so 34 i
// modulo 32 runs through the 16 even residues: 32 different 8-byte columns of the 64 four-byte banks, and the same for
// lanes 32 .. 63 (DESIGN.md 8k has the argument for the Gram pass's E + 2).
//
// Out.  Register q of lane l of a block is row 4 q + l / 16, column l % 16.  Each accumulator is rounded
// to fp32 once and goes through LDS (the factor area again, after a barrier; rows 80 floats apart), where row a is
// stored `shift` words in, shift = the row's first element's distance from the slot's 16-byte grid modulo 8.  Then
// eight lanes take a row: a lane reads a run of 8 consecutive elements with two 16-byte LDS reads, and the run is
// aligned in the slot by construction.  A run that lies wholly inside the row, the tile and the launch, in a launch
// whose slot and reference share a phase, loads g and stores x in 16-byte accesses; the runs over a row's two ends,
// over the ends of the range, and every run of a launch whose phases disagree go element by element, each element
// checked against the tile, the matrix and [idx0, idx0 + cnt).  A range may cut a matrix anywhere.
//
// Traffic: g is read once and x written once; the factors are read once per tile that uses them (128 r floats against
// 4096 outputs).  No atomics.  The loads of a tile's factors do not overlap its own MFMAs: a workgroup holds 34 KiB of
// LDS, so four of them share a CU and one's fill runs under another's matrix work and stores.
//
// Bit-exactness: `#pragma clang fp contract(off)`, every product exact in fp64, one rounding to fp32, one fp32 add;
// the order of the fp64 adds is not part of the rule.  Compiled without packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "fa_device.h"
#include "fa_host.h"
#include "fa_internal.h"
#include "fa_lowrank.h"
#include "fa_mx8.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

// The records, LrArgs, lr_run and lr_walk: fa_lowrank.h, shared with the low-rank-sum round.

// A rest chunk: lane t the runs t, t + 256, ... of the chunk's elements, the deltas straight from f.
template <typename DST, typename REF>
__device__ __forceinline__ void lr_rest(const LrArgs& a, const LrHeader* h, const LrRestRec& rc) {
    const int64_t i0 = (int64_t)(rc.start - a.idx0), i1 = i0 + rc.len;
    const float* fr = a.f + (uint64_t)a.r * h->total_rc + rc.fpos;
    const int64_t gb = i0 - mod8(i0 - a.hd);
    const int ng = (int)((i1 - gb + kLrRun - 1) / kLrRun);
    for (int m = threadIdx.x; m < ng; m += kLrThreads) {
        const int64_t base = gb + (int64_t)m * kLrRun;
        const int lo = (int)std::max<int64_t>(0, std::max(i0, (int64_t)0) - base);
        const int hi = (int)std::min<int64_t>(kLrRun, std::min(i1, a.cnt) - base);
        if (lo >= hi) continue;
        float d[kLrRun];
#pragma unroll
        for (int k = 0; k < kLrRun; ++k) d[k] = k >= lo && k < hi ? fr[base + k - i0] : 0.0f;
        lr_run<DST, REF>(a, base, lo, hi, d);
    }
}

template <typename DST, typename REF>
__global__ __launch_bounds__(kLrThreads) void lowrank_expand_kernel(const LrArgs a) {
    __shared__ __attribute__((aligned(16))) double fac[2 * kLrTile * kLrRs];  // P rows, then Q rows; later the results
    const LrHeader* h = reinterpret_cast<const LrHeader*>(a.plan);
    if (h->idx0 != a.idx0 || h->cnt != (uint64_t)a.cnt) return;  // a plan of another range
    const uint32_t blk = blockIdx.x;
    if (blk >= h->ntiles + h->nrest) return;
    if (blk >= h->ntiles) {
        lr_rest<DST, REF>(a, h, reinterpret_cast<const LrRestRec*>(h + 1)[blk]);
        return;
    }
    const LrTileRec tr = reinterpret_cast<const LrTileRec*>(h + 1)[blk];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int nrow = (int)std::min<uint32_t>(kLrTile, tr.rows - tr.row0), ncol = (int)std::min<uint32_t>(kLrTile, tr.cols - tr.col0);
    const uint32_t r = a.r;
    const float* fp = a.f + (uint64_t)r * (tr.pre + tr.row0);            // P's row row0
    const float* fq = a.f + (uint64_t)r * (tr.pre + tr.rows + tr.col0);  // Q's row col0
    const bool live = 16 * wave < nrow;  // uniform in a wave

    f64x4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[cb] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (uint32_t k0 = 0; k0 < r; k0 += kLrKc) {
        const int kc = (int)std::min<uint32_t>(kLrKc, (r - k0 + 3) & ~3u);  // this fill's rank, padded to 4
        if (k0) __syncthreads();                                           // the MFMAs of the fill before
        for (int e = threadIdx.x; e < 2 * kLrTile * kc; e += kLrThreads) {
            const int row = e / kc, t = e - row * kc;
            const bool q = row >= kLrTile;
            const int rr = q ? row - kLrTile : row;
            double v = 0.0;
            if (rr < (q ? ncol : nrow) && k0 + t < r) v = (double)(q ? fq : fp)[(uint64_t)rr * r + k0 + t];
            fac[row * kLrRs + t] = v;
        }
        __syncthreads();
        if (!live) continue;
        const double* pa = fac + (16 * wave + (lane & 15)) * kLrRs + (lane >> 4);
        const double* pb = fac + (kLrTile + (lane & 15)) * kLrRs + (lane >> 4);
        for (int s = 0; s < kc / 4; ++s) {
            const double x = pa[4 * s];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                if (16 * cb < ncol) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, pb[16 * cb * kLrRs + 4 * s], acc[cb], 0, 0, 0);
        }
    }
    __syncthreads();  // every wave has read its factors: the area takes the results

    float* out = reinterpret_cast<float*>(fac);
    // the slot element of the tile's (row 0, column 0), and of a row below it
    const int64_t e00 = (int64_t)(tr.off - a.idx0) + (int64_t)tr.row0 * tr.cols + tr.col0;
    if (live) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = 16 * wave + 4 * q + (lane >> 4);
            float* o = out + row * kLrOutRs + mod8(e00 + (int64_t)row * tr.cols - a.hd) + (lane & 15);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                if (16 * cb < ncol) o[16 * cb] = (float)acc[cb][q];
        }
    }
    __syncthreads();
    for (int row = threadIdx.x / kLrRun; row < nrow; row += kLrThreads / kLrRun) {
        const int64_t e0 = e00 + (int64_t)row * tr.cols;  // the row's first element of the tile, in the slot
        const int sh = mod8(e0 - a.hd);
        // the row's elements that the launch holds, as words [w0, w1) of its LDS row
        const int w0 = sh + (int)std::max<int64_t>(0, std::min<int64_t>(ncol, -e0));
        const int w1 = sh + (int)std::max<int64_t>(0, std::min<int64_t>(ncol, a.cnt - e0));
        for (int g = threadIdx.x % kLrRun; kLrRun * g < w1; g += kLrRun) {
            const int lo = std::max(0, w0 - kLrRun * g), hi = std::min(kLrRun, w1 - kLrRun * g);
            if (lo >= hi) continue;
            const f32x4* w = reinterpret_cast<const f32x4*>(out + row * kLrOutRs + kLrRun * g);
            const f32x4 u = w[0], v = w[1];
            float d[kLrRun] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
            lr_run<DST, REF>(a, e0 - sh + kLrRun * g, lo, hi, d);
        }
    }
}

template <typename DST, typename REF>
void launch_t(const LrArgs& a, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((lowrank_expand_kernel<DST, REF>), dim3(blocks), dim3(kLrThreads), 0, s, a);
}

template <typename DST>
void launch_d(const LrArgs& a, fa_dtype rdt, unsigned blocks, hipStream_t s) {
    if (!a.ref) {
        launch_t<DST, NoRef>(a, blocks, s);
    } else if (rdt == FA_F32) {
        launch_t<DST, float>(a, blocks, s);
    } else {  // a 16-bit reference: the slot's own type or an f32 slot (dtype_pair_ok)
        if constexpr (__is_same(DST, float)) {
            if (rdt == FA_BF16) launch_t<DST, uint16_t>(a, blocks, s);
            else launch_t<DST, _Float16>(a, blocks, s);
        } else {
            launch_t<DST, DST>(a, blocks, s);
        }
    }
}

struct LrPlan {
    LrHeader h;
    std::vector<LrTileRec> tiles;
    std::vector<LrRestRec> rest;
};

LrPlan lr_plan(const fa_lowrank_mat* mats, size_t M, uint64_t n, uint64_t idx0, uint64_t cnt) {
    LrPlan pl;
    const uint64_t end = idx0 + cnt;
    const uint64_t rc = lr_walk(
        mats, M, n,
        [&](size_t j, uint64_t pre) {
            const fa_lowrank_mat& m = mats[j];
            const uint64_t mend = m.off + (uint64_t)m.rows * m.cols;
            if (cnt == 0 || mend <= idx0 || m.off >= end) return;
            const uint64_t a0 = m.off >= idx0 ? 0 : (idx0 - m.off) / m.cols;  // the first and last row the range meets
            const uint64_t a1 = std::min<uint64_t>(m.rows - 1, (end - 1 - m.off) / m.cols);
            for (uint64_t tb = a0 / kLrTile; tb <= a1 / kLrTile; ++tb)
                for (uint64_t c0 = 0; c0 < m.cols; c0 += kLrTile)
                    pl.tiles.push_back(LrTileRec{m.off, pre, m.rows, m.cols, (uint32_t)(tb * kLrTile), (uint32_t)c0});
        },
        [&](uint64_t start, uint64_t len, uint64_t fpos) {
            const uint64_t s = std::max(start, idx0), e = std::min(start + len, end);
            for (uint64_t c = s; c < e; c += kLrRestChunk)
                pl.rest.push_back(LrRestRec{c, fpos + (c - start), (uint32_t)std::min<uint64_t>(kLrRestChunk, e - c), 0, 0});
        });
    pl.h = LrHeader{idx0, cnt, rc, (uint32_t)pl.tiles.size(), (uint32_t)pl.rest.size()};
    return pl;
}

}  // namespace

const char* lowrank_check(const fa_lowrank_mat* mats, size_t M, uint64_t n, size_t* bad) {
    uint64_t cur = 0;
    for (size_t j = 0; j < M; ++j) {
        const fa_lowrank_mat& m = mats[j];
        *bad = j;
        if (m.rows == 0 || m.cols == 0) return "has no rows or no columns";
        if (j && m.off < mats[j - 1].off) return "lies before its predecessor (entries ascend by off)";
        if (m.off < cur) return "overlaps its predecessor";
        if (m.off > n || (uint64_t)m.rows * m.cols > n - m.off) return "ends beyond the bucket";
        cur = m.off + (uint64_t)m.rows * m.cols;
    }
    return nullptr;
}

uint64_t lowrank_len(const fa_lowrank_mat* mats, size_t M, uint64_t n, int r) {
    uint64_t rest = 0;
    const uint64_t rc = lr_walk(mats, M, n, [](size_t, uint64_t) {}, [&](uint64_t, uint64_t len, uint64_t) { rest += len; });
    return (uint64_t)r * rc + rest;
}

size_t lowrank_plan_bytes(const fa_lowrank_mat* mats, size_t M, uint64_t n, uint64_t idx0, uint64_t cnt) {
    const LrPlan pl = lr_plan(mats, M, n, idx0, cnt);
    return sizeof(LrHeader) * (1 + pl.tiles.size() + pl.rest.size());
}

void lowrank_plan_build(const fa_lowrank_mat* mats, size_t M, uint64_t n, uint64_t idx0, uint64_t cnt, void* plan) {
    const LrPlan pl = lr_plan(mats, M, n, idx0, cnt);
    char* o = static_cast<char*>(plan);
    memcpy(o, &pl.h, sizeof pl.h);
    o += sizeof pl.h;
    if (!pl.tiles.empty()) memcpy(o, pl.tiles.data(), pl.tiles.size() * sizeof(LrTileRec));
    o += pl.tiles.size() * sizeof(LrTileRec);
    if (!pl.rest.empty()) memcpy(o, pl.rest.data(), pl.rest.size() * sizeof(LrRestRec));
}

// The decode rule on the host: ascending t, every product exact, one rounding.
void lowrank_decode_host(const fa_lowrank_mat* mats, size_t M, uint64_t n, const float* f, int r, uint64_t idx0, uint64_t cnt,
                         float* d) {
    const uint64_t end = idx0 + cnt;
    const uint64_t rc = lr_walk(mats, M, n, [](size_t, uint64_t) {}, [](uint64_t, uint64_t, uint64_t) {});
    const float* rest = f + (uint64_t)r * rc;
    lr_walk(
        mats, M, n,
        [&](size_t j, uint64_t pre) {
            const fa_lowrank_mat& m = mats[j];
            const float *P = f + (uint64_t)r * pre, *Q = P + (uint64_t)r * m.rows;
            const uint64_t s = std::max(m.off, idx0), e = std::min(m.off + (uint64_t)m.rows * m.cols, end);
            for (uint64_t i = s; i < e; ++i) {
                const uint64_t a = (i - m.off) / m.cols, b = (i - m.off) % m.cols;
                double S = 0.0;
                for (int t = 0; t < r; ++t) S += (double)P[a * r + t] * (double)Q[b * r + t];
                d[i - idx0] = (float)S;
            }
        },
        [&](uint64_t start, uint64_t len, uint64_t fpos) {
            for (uint64_t i = std::max(start, idx0); i < std::min(start + len, end); ++i) d[i - idx0] = rest[fpos + (i - start)];
        });
}

hipError_t launch_lowrank_expand(const void* plan, size_t plan_bytes, const float* f, int r, uint64_t idx0, int64_t cnt,
                                 const void* ref, fa_dtype rdt, void* dst, fa_dtype ddt, hipStream_t s) {
    if (cnt <= 0 || plan_bytes <= sizeof(LrHeader)) return hipSuccess;
    if (!plan || !f || !dst || r < 1 || r > FA_LOWRANK_MAX_RANK || (ref && !dtype_pair_ok(ddt, rdt))) return hipErrorInvalidValue;
    const size_t ds = ddt == FA_F32 ? 4 : 2, rs = rdt == FA_F32 ? 4 : 2;
    const int hd = (int)(((16 - (uintptr_t)dst % 16) % 16) / ds);
    const int vec = !ref || ((uintptr_t)ref + (size_t)hd * rs) % 16 == 0;
    const LrArgs a{plan, f, (uint32_t)r, idx0, cnt, ref, dst, hd, vec};
    const unsigned blocks = (unsigned)(plan_bytes / sizeof(LrHeader) - 1);
    switch (ddt) {
        case FA_F32: launch_d<float>(a, rdt, blocks, s); break;
        case FA_BF16: launch_d<uint16_t>(a, rdt, blocks, s); break;
        case FA_F16: launch_d<_Float16>(a, rdt, blocks, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fa

using namespace fah;

namespace {

// The checks every table entry point shares: the first bad entry by its index.
int check_table(const fa_lowrank_mat* mats, size_t M, size_t n) {
    if (M && !mats) return fail(FA_ERR_ARG, "lowrank: mats is null");
    size_t bad = 0;
    if (const char* why = fa::lowrank_check(mats, M, n, &bad))
        return fail(FA_ERR_ARG, "lowrank: matrix %zu (off %llu, %u x %u) %s; the bucket holds %zu elements", bad,
                    (unsigned long long)mats[bad].off, mats[bad].rows, mats[bad].cols, why, n);
    return FA_OK;
}
int check_range(uint64_t idx0, size_t cnt, size_t n) {
    if (idx0 + (uint64_t)cnt < idx0 || idx0 + (uint64_t)cnt > (uint64_t)n)
        return fail(FA_ERR_ARG, "lowrank: elements [%llu, + %zu) beyond the bucket's %zu", (unsigned long long)idx0, cnt, n);
    return FA_OK;
}
int check_rank(int r) {
    if (r < 1 || r > FA_LOWRANK_MAX_RANK) return fail(FA_ERR_ARG, "lowrank: rank %d outside 1 .. %d", r, FA_LOWRANK_MAX_RANK);
    return FA_OK;
}

}  // namespace

extern "C" {

int fa_lowrank_check(const fa_lowrank_mat* mats, size_t M, size_t n) {
    g_err.clear();
    return check_table(mats, M, n);
}

size_t fa_lowrank_len(const fa_lowrank_mat* mats, size_t M, size_t n, int r) {
    g_err.clear();
    if (check_table(mats, M, n) || check_rank(r)) return 0;
    return (size_t)fa::lowrank_len(mats, M, n, r);
}

int fa_lowrank_decode(const fa_lowrank_mat* mats, size_t M, size_t n, const float* f, int r, uint64_t idx0, size_t cnt,
                      float* d) {
    g_err.clear();
    if (int rc = check_table(mats, M, n)) return rc;
    if (int rc = check_rank(r)) return rc;
    if (int rc = check_range(idx0, cnt, n)) return rc;
    if (cnt == 0) return FA_OK;
    if (!f || !d) return fail(FA_ERR_ARG, "lowrank: %s is null", !f ? "f" : "d");
    fa::lowrank_decode_host(mats, M, n, f, r, idx0, cnt, d);
    return FA_OK;
}

size_t fa_lowrank_plan_bytes(const fa_lowrank_mat* mats, size_t M, size_t n, uint64_t idx0, size_t cnt) {
    g_err.clear();
    if (check_table(mats, M, n) || check_range(idx0, cnt, n)) return 0;
    return fa::lowrank_plan_bytes(mats, M, n, idx0, cnt);
}

int fa_lowrank_plan_build(const fa_lowrank_mat* mats, size_t M, size_t n, uint64_t idx0, size_t cnt, void* plan,
                          size_t plan_bytes) {
    g_err.clear();
    if (int rc = check_table(mats, M, n)) return rc;
    if (int rc = check_range(idx0, cnt, n)) return rc;
    if (!plan) return fail(FA_ERR_ARG, "lowrank: plan is null");
    const size_t need = fa::lowrank_plan_bytes(mats, M, n, idx0, cnt);
    if (plan_bytes != need) return fail(FA_ERR_ARG, "lowrank: the plan takes %zu bytes, %zu given (fa_lowrank_plan_bytes)", need, plan_bytes);
    fa::lowrank_plan_build(mats, M, n, idx0, cnt, plan);
    return FA_OK;
}

int fa_lowrank_expand_device(fa_ctx* ctx, int gpu, const void* d_plan, size_t plan_bytes, const float* d_f, int r,
                             uint64_t idx0, size_t cnt, const void* d_ref, fa_dtype ref_dtype, void* d_dst,
                             fa_dtype dst_dtype, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with cnt == 0 this is the feature probe of a box without a GPU
    if (!dvalid(dst_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (!fa::dtype_pair_ok(dst_dtype, ref_dtype))
        return fail(FA_ERR_ARG, "lowrank: no %s slot against a %s reference (a 16-bit slot takes its own type or f32)",
                    fa::dtype_name(dst_dtype), fa::dtype_name(ref_dtype));
    if (idx0 + (uint64_t)cnt < idx0) return fail(FA_ERR_ARG, "lowrank: idx0 + cnt beyond 2^64");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (cnt == 0) return FA_OK;
    if (int rc = check_rank(r)) return rc;
    if (!d_plan || !d_f || !d_dst)
        return fail(FA_ERR_ARG, "lowrank: %s pointer is null", !d_plan ? "d_plan" : !d_f ? "d_f" : "d_dst");
    if (plan_bytes < 32 || plan_bytes % 32)
        return fail(FA_ERR_ARG, "lowrank: %zu is no plan size (fa_lowrank_plan_bytes: a multiple of 32, at least 32)", plan_bytes);
    if (!aligned(d_plan, 8) || !aligned(d_f, 4))
        return fail(FA_ERR_ALIGN, "lowrank: %s", !aligned(d_plan, 8) ? "d_plan not 8-byte aligned" : "d_f not 4-byte aligned");
    if (d_ref && !aligned(d_ref, dsize(ref_dtype)))
        return fail(FA_ERR_ALIGN, "lowrank: reference not %zu-byte aligned", dsize(ref_dtype));
    if (!aligned(d_dst, dsize(dst_dtype))) return fail(FA_ERR_ALIGN, "lowrank: slot not %zu-byte aligned", dsize(dst_dtype));
    if (d_ref) {
        const uintptr_t o = (uintptr_t)d_dst, ob = (uintptr_t)(cnt * dsize(dst_dtype));
        const uintptr_t g = (uintptr_t)d_ref, gb = (uintptr_t)(cnt * dsize(ref_dtype));
        if (o < g + gb && g < o + ob) return fail(FA_ERR_ARG, "lowrank: d_dst overlaps d_ref");
    }
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_lowrank_expand(d_plan, plan_bytes, d_f, r, idx0, (int64_t)cnt, d_ref, ref_dtype, d_dst, dst_dtype, c.s));
    return FA_OK;
}

}  // extern "C"
