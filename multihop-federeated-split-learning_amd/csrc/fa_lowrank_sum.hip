// fa_lowrank_sum.hip -- the low-rank-sum stage (fa.h "Low-rank-sum stage") for CDNA4 (gfx950): a round of low-rank
// receipts reduced without expanding them.  The weighted sum of the owners' products is itself one product,
//   sum_c w_c P_c Q_c^T = [w_1 P_1 | ... | w_D P_D] [Q_1 | ... | Q_D]^T,
// so a tile of the aggregate is one GEMM over the stacked k-axis K = sum_c r_c (up to 8192), on the fp64 matrix unit as
// in fa_lowrank.hip: two widened fp32 values multiply exactly in fp64, the sum is rounded to fp32 once, g is read once
// and the output written once -- 8 bytes per element with fp32 g and output where the D expansions and the chain move
// about 12 D + 4.
//
// Plan.  The blob of lowrank_plan_build as it is (fa_lowrank.h): it does not depend on a rank.  One workgroup of 256
// lanes per record.  Its tile records are 64 x 64; a workgroup here takes a tile of 64 rows x 128 columns, the record
// with an even column tile and its right neighbour, and the workgroup of a record with an odd column tile returns at
// once (the planner lists a row band's column tiles back to back, and all of them).  The count behind the shape: per
// k-step of 4 a 64 x 64 tile reads 128 x 4 factor values from L2 for 4096 outputs, a 64 x 128 tile 192 x 4 for 8192:
// 0.031 K against 0.023 K floats per output, 25 % less; and a wave that owns 2 x 4 blocks reads 2 + 4 operands from LDS
// for 8 MFMAs (0.75 per MFMA) where the expansion's 1 x 4 reads 1 + 4 for 4 (1.25).  128 columns rather than 128 rows:
// the same counts, the two records of a tile are neighbours in the plan, and a row of results is 512 bytes of the
// output instead of 256.  The price is LDS: two buffers of 192 rows, one workgroup per CU (below).
//
// Stacked k-axis.  Every owner's rank is padded to a multiple of 4 with zeros, so a k-step of 4 belongs to one owner.
// The owners' pointers, ranks and weights travel in the kernel-argument segment as fa_mx8sum.hip's table does (2 KiB
// at 128 owners).  The k-step table (k-step -> owner, t0; at most 2048 entries) would not fit beside them in the 4 KiB
// of that segment, so each workgroup writes it into 4 KiB of LDS from the ranks: D wave-uniform steps, scalar loads.
//
// Pipelined k-loop.  A chunk is 32 stacked columns = 8 k-steps; LDS holds two chunk buffers of 64 P rows and 128 Q
// rows, 34 doubles apart (fa_lowrank.hip has the bank argument).  Wave w fills k-steps w and w + 4 of a chunk: the
// owner of a k-step is wave-uniform, so its pointer, rank and weight are scalar loads; lane l loads the 4 values of
// P row l and of Q rows l and l + 64 (24 floats in flight per lane), dead rows and the rank's padding as zeros.  Per
// chunk i: issue the global loads of chunk i + 1; the MFMAs of chunk i from buffer i % 2; then the rule-1 multiply
// fl32(w p), the widening to double and the LDS stores of chunk i + 1 into the other buffer; one barrier.  (The barrier
// orders both the stores before the next chunk's reads and this chunk's reads before the stores after the next.)
// Wave (wr, wc) owns rows 32 wr .. + 32 and columns 64 wc .. + 64 of the tile: 2 x 4 blocks, 32 accumulator doubles per
// lane that live across the whole loop; bands and blocks wholly past the matrix edge are skipped.
//
// Out.  As fa_lowrank.hip: each accumulator rounded once, through LDS (the buffers again; rows 144 floats apart) with
// the row shifted onto the output's 16-byte grid, then lr_run: 16-byte loads of g and stores where a run is whole,
// element by element at the edges and where the phases disagree.  Rest chunks run rule 3, the fmaf chain in client
// order over the owners' rest values, into the same lr_run.  No atomics.
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950, every dtype pair): 74 VGPRs, 64 AGPRs, 108544 bytes of
// LDS, no scratch, no spills, 1 wave per SIMD.  Measured: 0.23 - 0.79 of the expanded route's device time
// at r = 4 and 16, 1.03 - 1.08 at r = 64; the k-loop reaches 15.9 Tflop/s at D = 32, r = 64 where the unpipelined
// expansion reaches 17.8: with one wave per SIMD the LDS reads of a k-step are not hidden under the MFMAs before it.
//
// Bit-exactness: `#pragma clang fp contract(off)`: one fp32 multiply (rule 1), exact fp64 products, one rounding, one
// fp32 add; the fmaf of rule 3 is written as one.  Compiled without packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "fa_device.h"
#include "fa_host.h"
#include "fa_internal.h"
#include "fa_lowrank.h"
#include "fa_mx8.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kSumCols = 2 * kLrTile;                 // the columns of a tile: two records of the plan
constexpr int kSumRows = kLrTile + kSumCols;          // the rows of a chunk buffer: 64 of P, then 128 of Q
constexpr int kSumBuf = kSumRows * kLrRs;             // its doubles
constexpr int kSumSteps = kLrKc / 4;                  // the k-steps of a chunk
constexpr int kSumMaxSteps = kMaxClients * (FA_LOWRANK_MAX_RANK / 4);  // of a round: 2048
constexpr int kSumOutRs = kSumCols + 2 * kLrRun;      // floats between two result rows
static_assert(kSumSteps == 2 * kLrWaves, "a wave fills two k-steps of a chunk");
static_assert(kLrTile * kSumOutRs * sizeof(float) <= 2 * kSumBuf * sizeof(double), "the results fit the buffers");
static_assert(FA_LOWRANK_SUM_MAX_CLIENTS == kMaxClients && FA_LOWRANK_MAX_RANK / 4 <= 16, "owner << 4 | t0 / 4 in 16 bits");

// An owner's receipt, weight and rank side by side, 16 bytes: one scalar load, and every address into the table is a
// multiple of 4 (a byte array of ranks beside 8-byte pointers made the compiler split 8 c into c + 7 c across the base
// and the offset of a scalar load, which reads dword-aligned).
struct LrSumOwner {
    const float* f;
    float w;
    uint32_t r;
};
struct LrSumTable {  // 2 KiB of the kernel-argument segment
    LrSumOwner o[kMaxClients];
    int D;
};
static_assert(sizeof(LrSumOwner) == 16, "one 16-byte scalar load per owner");

// What a lane holds of the chunk being loaded: k-steps wave and wave + 4, rows P lane, Q lane, Q lane + 64.
struct LrSumFetch {
    float v[2][3][4];
    float w[2];
};

// The global loads of chunk `chunk` (nks: the k-steps of the round).  pr, q0, q1: the lane's rows as positions in a
// receipt of rank 1 (the row index among all factor rows), or -1 for a dead row.
__device__ __forceinline__ void lrs_fetch(const LrSumTable& tb, const uint16_t* ktab, int nks, int chunk, int wave, int64_t pr,
                                          int64_t q0, int64_t q1, LrSumFetch& x) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int s = kSumSteps * chunk + wave + kLrWaves * u;  // wave-uniform
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) x.v[u][m][j] = 0.0f;
        x.w[u] = 0.0f;
        if (s >= nks) continue;
        const int e = __builtin_amdgcn_readfirstlane((int)ktab[s]);
        const int c = e >> 4, t0 = (e & 15) * 4;
        const LrSumOwner ow = tb.o[c];
        const int rc = (int)ow.r;
        const float* fc = ow.f + t0;
        x.w[u] = ow.w;
        const int64_t row[3] = {pr, q0, q1};
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            if (row[m] < 0) continue;
            const float* p = fc + row[m] * rc;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t0 + j < rc) x.v[u][m][j] = p[j];
        }
    }
}

// Rule 1, the widening and the LDS stores of what lrs_fetch loaded.
__device__ __forceinline__ void lrs_commit(double* buf, int nks, int chunk, int wave, int lane, const LrSumFetch& x) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int sl = wave + kLrWaves * u;
        if (kSumSteps * chunk + sl >= nks) continue;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            double* o = buf + (lane + 64 * m) * kLrRs + 4 * sl;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = m == 0 ? (double)(x.w[u] * x.v[u][0][j]) : (double)x.v[u][m][j];
        }
    }
}

// A rest chunk, rule 3: lane t the runs t, t + 256, ... of the chunk's elements, the chain over the owners' rest values.
template <typename DST, typename REF>
__device__ __forceinline__ void lrs_rest(const LrSumTable& tb, const LrArgs& a, const LrHeader* h, const LrRestRec& rc) {
    const int64_t i0 = (int64_t)(rc.start - a.idx0), i1 = i0 + rc.len;
    const int64_t gb = i0 - mod8(i0 - a.hd);
    const int ng = (int)((i1 - gb + kLrRun - 1) / kLrRun);
    for (int m = threadIdx.x; m < ng; m += kLrThreads) {
        const int64_t base = gb + (int64_t)m * kLrRun;
        const int lo = (int)std::max<int64_t>(0, std::max(i0, (int64_t)0) - base);
        const int hi = (int)std::min<int64_t>(kLrRun, std::min(i1, a.cnt) - base);
        if (lo >= hi) continue;
        float acc[kLrRun];
#pragma unroll
        for (int k = 0; k < kLrRun; ++k) acc[k] = 0.0f;
        for (int c = 0; c < tb.D; ++c) {  // uniform: the table is read by scalar loads
            const LrSumOwner ow = tb.o[c];
            const float* fr = ow.f + (uint64_t)ow.r * h->total_rc + rc.fpos + (base - i0);
            const float w = ow.w;
#pragma unroll
            for (int k = 0; k < kLrRun; ++k)
                if (k >= lo && k < hi) acc[k] = __builtin_fmaf(w, fr[k], acc[k]);
        }
        lr_run<DST, REF>(a, base, lo, hi, acc);
    }
}

template <typename DST, typename REF>
__global__ __launch_bounds__(kLrThreads) void lowrank_sum_kernel(const LrSumTable tb, const LrArgs a) {
    __shared__ __attribute__((aligned(16))) double fac[2 * kSumBuf];  // two chunk buffers; later the results
    __shared__ uint16_t ktab[kSumMaxSteps];                          // k-step -> owner << 4 | t0 / 4
    const LrHeader* h = reinterpret_cast<const LrHeader*>(a.plan);
    if (h->idx0 != a.idx0 || h->cnt != (uint64_t)a.cnt) return;  // a plan of another range
    const uint32_t blk = blockIdx.x;
    if (blk >= h->ntiles + h->nrest) return;
    if (blk >= h->ntiles) {
        lrs_rest<DST, REF>(tb, a, h, reinterpret_cast<const LrRestRec*>(h + 1)[blk]);
        return;
    }
    const LrTileRec tr = reinterpret_cast<const LrTileRec*>(h + 1)[blk];
    if ((tr.col0 / kLrTile) & 1u) return;  // the right half of its left neighbour's tile
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave >> 1, wc = wave & 1;
    const int nrow = (int)std::min<uint32_t>(kLrTile, tr.rows - tr.row0), ncol = (int)std::min<uint32_t>(kSumCols, tr.cols - tr.col0);

    int nks = 0;
    for (int c = 0; c < tb.D; ++c) {  // uniform
        const int nk = (int)(tb.o[c].r + 3) >> 2;
        if (tid < nk) ktab[nks + tid] = (uint16_t)(c << 4 | tid);
        nks += nk;
    }
    __syncthreads();
    const int nch = (nks + kSumSteps - 1) / kSumSteps;

    // the lane's three rows among the factor rows of a receipt: P's row row0 + lane, Q's rows col0 + lane (+ 64)
    const int64_t pr = lane < nrow ? (int64_t)(tr.pre + tr.row0) + lane : -1;
    const int64_t q0 = lane < ncol ? (int64_t)(tr.pre + tr.rows + tr.col0) + lane : -1;
    const int64_t q1 = lane + 64 < ncol ? (int64_t)(tr.pre + tr.rows + tr.col0) + lane + 64 : -1;
    const bool band[2] = {32 * wr < nrow, 32 * wr + 16 < nrow};  // uniform in a wave

    f64x4 acc[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[b][cb] = f64x4{0.0, 0.0, 0.0, 0.0};

    LrSumFetch x;
    lrs_fetch(tb, ktab, nks, 0, wave, pr, q0, q1, x);
    lrs_commit(fac, nks, 0, wave, lane, x);
    __syncthreads();
    for (int i = 0; i < nch; ++i) {
        const bool more = i + 1 < nch;
        if (more) lrs_fetch(tb, ktab, nks, i + 1, wave, pr, q0, q1, x);  // in flight under the MFMAs
        const double* buf = fac + (i & 1) * kSumBuf;
        if (band[0]) {
            const double* pa = buf + (32 * wr + (lane & 15)) * kLrRs + (lane >> 4);
            const double* pb = buf + (kLrTile + 64 * wc + (lane & 15)) * kLrRs + (lane >> 4);
            const int ns = std::min(kSumSteps, nks - kSumSteps * i);
            for (int s = 0; s < ns; ++s) {
                const double a0 = pa[4 * s], a1 = pa[16 * kLrRs + 4 * s];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    if (64 * wc + 16 * cb >= ncol) continue;
                    const double y = pb[16 * cb * kLrRs + 4 * s];
                    acc[0][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, y, acc[0][cb], 0, 0, 0);
                    if (band[1]) acc[1][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, y, acc[1][cb], 0, 0, 0);
                }
            }
        }
        if (more) lrs_commit(fac + ((i + 1) & 1) * kSumBuf, nks, i + 1, wave, lane, x);
        __syncthreads();  // the one barrier of a chunk; after the last, the area takes the results
    }

    float* out = reinterpret_cast<float*>(fac);
    // the output element of the tile's (row 0, column 0), and of a row below it
    const int64_t e00 = (int64_t)(tr.off - a.idx0) + (int64_t)tr.row0 * tr.cols + tr.col0;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (!band[b]) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = 32 * wr + 16 * b + 4 * q + (lane >> 4);
            float* o = out + row * kSumOutRs + mod8(e00 + (int64_t)row * tr.cols - a.hd) + 64 * wc + (lane & 15);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                if (64 * wc + 16 * cb < ncol) o[16 * cb] = (float)acc[b][cb][q];
        }
    }
    __syncthreads();
    for (int row = tid / kLrRun; row < nrow; row += kLrThreads / kLrRun) {
        const int64_t e0 = e00 + (int64_t)row * tr.cols;  // the row's first element of the tile, in the output
        const int sh = mod8(e0 - a.hd);
        // the row's elements that the launch holds, as words [w0, w1) of its LDS row
        const int w0 = sh + (int)std::max<int64_t>(0, std::min<int64_t>(ncol, -e0));
        const int w1 = sh + (int)std::max<int64_t>(0, std::min<int64_t>(ncol, a.cnt - e0));
        for (int g = tid % kLrRun; kLrRun * g < w1; g += kLrRun) {
            const int lo = std::max(0, w0 - kLrRun * g), hi = std::min(kLrRun, w1 - kLrRun * g);
            if (lo >= hi) continue;
            const f32x4* w = reinterpret_cast<const f32x4*>(out + row * kSumOutRs + kLrRun * g);
            const f32x4 u = w[0], v = w[1];
            float d[kLrRun] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
            lr_run<DST, REF>(a, e0 - sh + kLrRun * g, lo, hi, d);
        }
    }
}

template <typename DST, typename REF>
void launch_t(const LrSumTable& tb, const LrArgs& a, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((lowrank_sum_kernel<DST, REF>), dim3(blocks), dim3(kLrThreads), 0, s, tb, a);
}

template <typename DST>
void launch_d(const LrSumTable& tb, const LrArgs& a, fa_dtype rdt, unsigned blocks, hipStream_t s) {
    if (!a.ref) {
        launch_t<DST, NoRef>(tb, a, blocks, s);
    } else if (rdt == FA_F32) {
        launch_t<DST, float>(tb, a, blocks, s);
    } else {  // a 16-bit reference: the output's own type or an f32 output (dtype_pair_ok)
        if constexpr (__is_same(DST, float)) {
            if (rdt == FA_BF16) launch_t<DST, uint16_t>(tb, a, blocks, s);
            else launch_t<DST, _Float16>(tb, a, blocks, s);
        } else {
            launch_t<DST, DST>(tb, a, blocks, s);
        }
    }
}

}  // namespace

hipError_t launch_lowrank_sum(const void* plan, size_t plan_bytes, const float* const* f, const int* r, const float* w, int D,
                              uint64_t idx0, int64_t cnt, const void* ref, fa_dtype rdt, void* out, fa_dtype odt, hipStream_t s) {
    if (cnt <= 0 || plan_bytes <= sizeof(LrHeader)) return hipSuccess;
    if (!plan || !f || !r || !w || !out || D < 1 || D > kMaxClients || (ref && !dtype_pair_ok(odt, rdt))) return hipErrorInvalidValue;
    LrSumTable tb;
    tb.D = D;
    for (int c = 0; c < kMaxClients; ++c) {
        const bool in = c < D;
        if (in && (!f[c] || r[c] < 1 || r[c] > FA_LOWRANK_MAX_RANK)) return hipErrorInvalidValue;
        tb.o[c] = in ? LrSumOwner{f[c], w[c], (uint32_t)r[c]} : LrSumOwner{nullptr, 0.0f, 0};
    }
    const size_t ds = odt == FA_F32 ? 4 : 2, rs = rdt == FA_F32 ? 4 : 2;
    const int hd = (int)(((16 - (uintptr_t)out % 16) % 16) / ds);
    const int vec = !ref || ((uintptr_t)ref + (size_t)hd * rs) % 16 == 0;
    const LrArgs a{plan, nullptr, 0, idx0, cnt, ref, out, hd, vec};
    const unsigned blocks = (unsigned)(plan_bytes / sizeof(LrHeader) - 1);
    switch (odt) {
        case FA_F32: launch_d<float>(tb, a, rdt, blocks, s); break;
        case FA_BF16: launch_d<uint16_t>(tb, a, rdt, blocks, s); break;
        case FA_F16: launch_d<_Float16>(tb, a, rdt, blocks, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// Rules 1-4 on the host: on a matrix the products in ascending (c, t), elsewhere the chain in ascending c.
void lowrank_sum_host(const fa_lowrank_mat* mats, size_t M, uint64_t n, const float* const* f, const int* r, const float* w,
                      int D, uint64_t idx0, uint64_t cnt, const float* ref, float* out) {
#pragma clang fp contract(off)
    const uint64_t end = idx0 + cnt;
    const uint64_t rc = lr_walk(mats, M, n, [](size_t, uint64_t) {}, [](uint64_t, uint64_t, uint64_t) {});
    lr_walk(
        mats, M, n,
        [&](size_t j, uint64_t pre) {
            const fa_lowrank_mat& m = mats[j];
            const uint64_t s = std::max(m.off, idx0), e = std::min(m.off + (uint64_t)m.rows * m.cols, end);
            for (uint64_t i = s; i < e; ++i) {
                const uint64_t a = (i - m.off) / m.cols, b = (i - m.off) % m.cols;
                double S = 0.0;
                for (int c = 0; c < D; ++c) {
                    const float *P = f[c] + (uint64_t)r[c] * pre, *Q = P + (uint64_t)r[c] * m.rows;
                    for (int t = 0; t < r[c]; ++t) {
                        const float pw = w[c] * P[a * r[c] + t];
                        S += (double)pw * (double)Q[b * r[c] + t];
                    }
                }
                out[i - idx0] = (float)S;
            }
        },
        [&](uint64_t start, uint64_t len, uint64_t fpos) {
            for (uint64_t i = std::max(start, idx0); i < std::min(start + len, end); ++i) {
                float acc = 0.0f;
                for (int c = 0; c < D; ++c) acc = std::fmaf(w[c], f[c][(uint64_t)r[c] * rc + fpos + (i - start)], acc);
                out[i - idx0] = acc;
            }
        });
    for (uint64_t i = 0; ref && i < cnt; ++i) out[i] = ref[i] + out[i];
}

}  // namespace fa

using namespace fah;

namespace {

// What fa_lowrank_sum_host and fa_lowrank_sum_device refuse about the receipts before they look at a pointer's target.
int check_lowrank_sum(const float* const* f, const int* r, const float* w, int D, uint64_t idx0, size_t cnt) {
    if (D < 1 || D > FA_LOWRANK_SUM_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "lowrank sum: D = %d clients outside 1 .. %d", D, FA_LOWRANK_SUM_MAX_CLIENTS);
    if (idx0 + (uint64_t)cnt < idx0) return fail(FA_ERR_ARG, "lowrank sum: idx0 + cnt beyond 2^64");
    if (cnt == 0) return FA_OK;
    if (!f || !r || !w) return fail(FA_ERR_ARG, "lowrank sum: %s is null", !f ? "f" : !r ? "r" : "w");
    for (int c = 0; c < D; ++c) {
        if (r[c] < 1 || r[c] > FA_LOWRANK_MAX_RANK)
            return fail(FA_ERR_ARG, "lowrank sum: client %d's rank %d outside 1 .. %d", c, r[c], FA_LOWRANK_MAX_RANK);
        if (!f[c]) return fail(FA_ERR_ARG, "lowrank sum: client %d's f is null", c);
        if (!aligned(f[c], 4)) return fail(FA_ERR_ALIGN, "lowrank sum: client %d's f not 4-byte aligned", c);
    }
    return FA_OK;
}

}  // namespace

extern "C" {

int fa_lowrank_sum_host(const fa_lowrank_mat* mats, size_t M, size_t n, const float* const* f, const int* r, const float* w,
                        int D, uint64_t idx0, size_t cnt, const float* ref, float* out) {
    g_err.clear();
    if (int rc = fa_lowrank_check(mats, M, n)) return rc;
    if (int rc = check_lowrank_sum(f, r, w, D, idx0, cnt)) return rc;
    if (idx0 + (uint64_t)cnt > (uint64_t)n)
        return fail(FA_ERR_ARG, "lowrank sum: elements [%llu, + %zu) beyond the bucket's %zu", (unsigned long long)idx0, cnt, n);
    if (cnt == 0) return FA_OK;
    if (!out) return fail(FA_ERR_ARG, "lowrank sum: out is null");
    fa::lowrank_sum_host(mats, M, n, f, r, w, D, idx0, cnt, ref, out);
    return FA_OK;
}

int fa_lowrank_sum_device(fa_ctx* ctx, int gpu, const void* d_plan, size_t plan_bytes, const float* const* d_f, const int* r,
                          const float* w, int D, uint64_t idx0, size_t cnt, const void* d_ref, fa_dtype ref_dtype, void* d_out,
                          fa_dtype out_dtype, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with cnt == 0 this is the feature probe of a box without a GPU
    if (!dvalid(out_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (!fa::dtype_pair_ok(out_dtype, ref_dtype))
        return fail(FA_ERR_ARG, "lowrank sum: no %s output against a %s reference (a 16-bit output takes its own type or f32)",
                    fa::dtype_name(out_dtype), fa::dtype_name(ref_dtype));
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (int rc = check_lowrank_sum(d_f, r, w, D, idx0, cnt)) return rc;
    if (cnt == 0) return FA_OK;
    if (!d_plan || !d_out) return fail(FA_ERR_ARG, "lowrank sum: %s pointer is null", !d_plan ? "d_plan" : "d_out");
    if (plan_bytes < 32 || plan_bytes % 32)
        return fail(FA_ERR_ARG, "lowrank sum: %zu is no plan size (fa_lowrank_plan_bytes: a multiple of 32, at least 32)", plan_bytes);
    if (!aligned(d_plan, 8)) return fail(FA_ERR_ALIGN, "lowrank sum: d_plan not 8-byte aligned");
    if (d_ref && !aligned(d_ref, dsize(ref_dtype)))
        return fail(FA_ERR_ALIGN, "lowrank sum: reference not %zu-byte aligned", dsize(ref_dtype));
    if (!aligned(d_out, dsize(out_dtype))) return fail(FA_ERR_ALIGN, "lowrank sum: output not %zu-byte aligned", dsize(out_dtype));
    if (d_ref) {
        const uintptr_t o = (uintptr_t)d_out, ob = (uintptr_t)(cnt * dsize(out_dtype));
        const uintptr_t g = (uintptr_t)d_ref, gb = (uintptr_t)(cnt * dsize(ref_dtype));
        if (o < g + gb && g < o + ob) return fail(FA_ERR_ARG, "lowrank sum: d_out overlaps d_ref");
    }
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_lowrank_sum(d_plan, plan_bytes, d_f, r, w, D, idx0, (int64_t)cnt, d_ref, ref_dtype, d_out, out_dtype, c.s));
    return FA_OK;
}

}  // extern "C"
