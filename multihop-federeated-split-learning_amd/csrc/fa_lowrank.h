// fa_lowrank.h -- what the two low-rank kernels share (fa_lowrank.hip: a receipt expanded into a slot; fa_lowrank_sum.hip:
// a round of receipts reduced as one stacked product): the plan blob's records, the walk over a part's table, and the
// store of a run of 8 results laid on the output's 16-byte grid.  Included by those two files only; everything here has
// internal linkage on purpose (the kernels are templates over NoRef).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"
#include "fa_mx8.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kLrThreads = 256, kLrWaves = kLrThreads / 64;
constexpr int kLrTile = 64;                      // rows and columns of an output tile: 4 x 4 blocks of 16 x 16
constexpr int kLrKc = 32, kLrRs = kLrKc + 2;     // the rank per fill, and the doubles between two factor rows
constexpr int kLrRun = 8;                        // the elements of a lane's run: 16 bytes of a 16-bit slot, 32 of fp32
constexpr int kLrOutRs = kLrTile + 2 * kLrRun;   // floats between two result rows: 64 + the shift (< 8), 16-byte rows
constexpr int kLrRestChunk = kLrThreads * kLrRun;
static_assert(kLrTile == 16 * kLrWaves && kLrRs % 4 == 2, "a wave per 16-row band; rows 2 x odd doubles apart");
static_assert(kLrTile * kLrOutRs * sizeof(float) <= 2 * kLrTile * kLrRs * sizeof(double), "the results fit the factors' LDS");

// The plan blob: LrHeader, ntiles LrTileRec, nrest LrRestRec; 32 bytes each.
struct LrHeader {
    uint64_t idx0, cnt;    // the range it was built for: a launch over another range does nothing
    uint64_t total_rc;     // sum_j (rows_j + cols_j) over the whole table: rest lies r * total_rc floats into f
    uint32_t ntiles, nrest;
};
struct LrTileRec {
    uint64_t off, pre;     // the matrix's first bucket element; the rows and columns of the matrices before it
    uint32_t rows, cols, row0, col0;
};
struct LrRestRec {
    uint64_t start, fpos;  // the chunk's first bucket element, and its position among the rest values
    uint32_t len, pad0;
    uint64_t pad1;
};
static_assert(sizeof(LrHeader) == 32 && sizeof(LrTileRec) == 32 && sizeof(LrRestRec) == 32, "32-byte records");

struct NoRef {};

struct LrArgs {
    const void* plan;
    const float* f;  // the expansion's receipt and rank (the sum stage has a table of them: null and 0 there)
    uint32_t r;
    uint64_t idx0;
    int64_t cnt;
    const void* ref;
    void* dst;
    int hd;   // the elements from dst to its first 16-byte boundary: runs start at hd modulo 8
    int vec;  // the reference is 16-byte aligned there too: whole runs take 16-byte accesses
};

__device__ __forceinline__ int mod8(int64_t x) { return (int)((uint64_t)x & 7u); }

// Elements [lo, hi) of the run of 8 at slot element i (i = hd modulo 8; lo > 0 where i < 0): x = g + d, or d.
template <typename DST, typename REF>
__device__ __forceinline__ void lr_run(const LrArgs& a, int64_t i, int lo, int hi, float* d) {
    if (a.vec && lo == 0 && hi == kLrRun) {
        if constexpr (!__is_same(REF, NoRef)) {
            float g[kLrRun];
            const REF* p = reinterpret_cast<const REF*>(a.ref) + i;
#pragma unroll
            for (int j = 0; j < kLrRun; j += In<REF>::kVec) In<REF>::widen(ld16<false>(p + j), g + j);
#pragma unroll
            for (int j = 0; j < kLrRun; ++j) d[j] = mx8_add(g[j], d[j]);
        }
        Out<DST>::template store<kLrRun, kStPlain>(a.dst, i, d);
        return;
    }
#pragma unroll
    for (int k = 0; k < kLrRun; ++k) {
        if (k < lo || k >= hi) continue;
        float x = d[k];
        if constexpr (!__is_same(REF, NoRef)) x = mx8_add(In<REF>::scalar(a.ref, i + k), x);
        Out<DST>::scalar(a.dst, i + k, x);
    }
}

// The table walked in bucket order: mat(j, pre) for every matrix with the rows and columns before it, gap(start, len,
// fpos) for every non-empty run of rest elements with the rest elements before it.  Returns sum_j (rows_j + cols_j).
template <class Mat, class Gap>
uint64_t lr_walk(const fa_lowrank_mat* mats, size_t M, uint64_t n, Mat mat, Gap gap) {
    uint64_t cur = 0, pre = 0, fpos = 0;
    for (size_t j = 0; j <= M; ++j) {
        const uint64_t next = j < M ? mats[j].off : n;
        if (next > cur) gap(cur, next - cur, fpos);
        fpos += next - cur;
        if (j == M) break;
        mat(j, pre);
        pre += (uint64_t)mats[j].rows + mats[j].cols;
        cur = next + (uint64_t)mats[j].rows * mats[j].cols;
    }
    return pre;
}

}  // namespace

}  // namespace fa
