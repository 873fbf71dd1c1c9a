// fa_split.h -- how one launch splits a bucket between a kernel's vector form (16-byte loads of V = 16 / input
// element size elements) and its element form.  n elements are a head [0, head), nvec vectors [head, tail0) and
// a tail [tail0, n): the head brings the lead operand (the first client; FA_LITERAL's last; the optimizer's
// aggregate) to a 16-byte boundary, and the vector form is taken only if every other operand allows it.
// The rule, for an operand q of element size es (q es-aligned) after h head elements, V es being its bytes per
// input vector (32, fp32 beside 16-bit inputs, is two 16-byte accesses; 8 is a 16-bit output of fp32 inputs):
//     (q + h es) % min(16, V es) == 0
// The four spellings this type replaced are instances of it:
//   a further input, (q % 16) / si == phase:  es = si, h = (V - phase) % V: q + h si = 0 (16) <=> q / si = phase (V);
//   the output, (dst + head so) % min(16, V so):  the rule as it stands;
//   the optimizer's output, % (4 so):  V = 4 and 4 so <= 16;
//   init, the clip reference, the fp32 scratch, (p + head 4) % 16:  es = 4 and V 4 >= 16.
// One wrinkle is kept: a bucket that ends before the lead's boundary (n < lead) has head = n and no vector, and
// there inputs were still judged by their phase (h = lead), every other operand after the clamped head
// (h = head).  require_input and require keep both, so such a bucket takes the kernel it always took; for
// n >= lead they are one test.  Host-only, no HIP: the CPU suite tests it (tests/tools/split_selftest.cpp), and
// measure_grid below, the grid of the two measure passes over a Split (tests/tools/grid_selftest.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fa {

struct Split {
    int64_t head, nvec, n;  // elements before the first vector, whole vectors, all elements
    int V;                  // elements per 16-byte input vector
    int64_t lead;           // head before its clamp to n: elements from the lead operand to its 16-byte boundary
    bool vec;               // every operand required so far allows the vector form
    int64_t tail0() const { return head + nvec * V; }
    int64_t edges() const { return head + (n - tail0()); }  // elements left to the element form
    bool valid() const { return head >= 0 && nvec >= 0 && tail0() <= n; }  // else every launch_* refuses it
    void require_input(const void* p) { vec = vec && after(p, lead, (size_t)(16 / V)); }  // a further input
    void require(const void* p, size_t elem) { vec = vec && after(p, head, elem); }        // any other operand
    bool after(const void* p, int64_t h, size_t elem) const {
        const size_t width = (size_t)V * elem < 16 ? (size_t)V * elem : 16;
        return ((uintptr_t)p + (size_t)h * elem) % width == 0;
    }
};

// The split of n elements of size `elem` (2 or 4) led by `lead`, which alone allows the vector form.
inline Split split_at(const void* lead, size_t elem, size_t n) {
    const int V = (int)(16 / elem);
    const int64_t to16 = (int64_t)(((size_t)V - ((uintptr_t)lead % 16) / elem) % (size_t)V);
    const int64_t head = to16 < (int64_t)n ? to16 : (int64_t)n;
    return Split{head, ((int64_t)n - head) / V, (int64_t)n, V, to16, true};
}

// The grid of a measure pass (fa_clip.hip, fa_krum.hip) over sp in tiles of `tile` elements (a multiple of V):
// one workgroup per tile up to `cap`, the stage's own cap lowered by Tuning::max_blocks if that is > 0, the
// tiles beyond it strided.  With a vector part the vector kernel takes its tiles and one workgroup of the
// element kernel the edges, if any; else the element kernel takes all n elements.  np: the partials the pass
// writes per result, one per workgroup.
struct MeasureGrid {
    int64_t vec_blocks, elem_blocks;
    int64_t np() const { return vec_blocks + elem_blocks; }
};
inline MeasureGrid measure_grid(const Split& sp, int64_t tile, int64_t cap, int max_blocks) {
    if (max_blocks > 0 && max_blocks < cap) cap = max_blocks;
    const auto blocks = [cap](int64_t n, int64_t per) {
        const int64_t tiles = (n + per - 1) / per;
        return tiles < 1 ? 1 : tiles < cap ? tiles : cap;
    };
    if (sp.vec && sp.nvec > 0) return MeasureGrid{blocks(sp.nvec, tile / sp.V), sp.edges() > 0 ? 1 : 0};
    return MeasureGrid{0, blocks(sp.n, tile)};
}

}  // namespace fa
