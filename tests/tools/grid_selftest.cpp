// grid_selftest.cpp -- CPU test of the grid of a measure pass (fa::measure_grid, csrc/fa_split.h).
//
// measure_grid replaced two hand-written copies of one computation: ClipGrid / clip_grid / blocks_of in
// fa_clip.hip and blocks_of with the head of launch_pairdist_t in fa_krum.hip.  This program keeps both, verbatim
// with their constants, as the legacy_* functions below and compares the function with them: both input element
// sizes (V = 4 and 8), the lead on and off a 16-byte boundary, the vector form allowed and refused (mixed
// phases), six values of Tuning::max_blocks around the stages' caps, and thirteen n around one tile, two tiles
// and the cap -- for the clip stage's tile of 4096 elements and the Krum stage's E at D = 3, 33 and 128 (E from
// krum_geom's rule, copied as well).  A handful of cases then pin the numbers themselves.  Addresses are made
// from integers and never dereferenced.  tests/test_host_sanitizers.py computes the number of checks from the
// same ranges.  Last line: one JSON line; exit code 1 if any check failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "fa_split.h"

namespace {

int checks = 0, failed = 0;
void check(bool ok, const char* what, int V, int64_t tile, int64_t n, int max_blocks, bool vec, size_t phase) {
    ++checks;
    if (ok) return;
    ++failed;
    if (failed <= 20)
        std::fprintf(stderr, "FAIL %s: V %d tile %lld n %lld max_blocks %d vec %d phase %zu\n", what, V, (long long)tile,
                     (long long)n, max_blocks, (int)vec, phase);
}

using fa::Split;
struct Tuning {
    int max_blocks;
};

// ---- fa_clip.hip as it stood
constexpr int kClipThreads = 256;
constexpr int kClipLaneElems = 16;
constexpr int64_t kClipTile = (int64_t)kClipThreads * kClipLaneElems;
constexpr int64_t kClipMaxBlocks = 2048;
int64_t clip_blocks_of(int64_t tiles, const Tuning& tu) {
    int64_t cap = kClipMaxBlocks;
    if (tu.max_blocks > 0) cap = std::min<int64_t>(cap, tu.max_blocks);
    return std::max<int64_t>(1, std::min(tiles, cap));
}
struct ClipGrid {
    int64_t vec_blocks, elem_blocks;
};
ClipGrid clip_grid(const Split& sp, const Tuning& tu) {
    if (sp.vec && sp.nvec > 0) {
        const int64_t tile_vecs = kClipTile / sp.V;
        return ClipGrid{clip_blocks_of((sp.nvec + tile_vecs - 1) / tile_vecs, tu), sp.edges() > 0 ? 1 : 0};
    }
    return ClipGrid{0, clip_blocks_of((sp.n + kClipTile - 1) / kClipTile, tu)};
}

// ---- fa_krum.hip as it stood: E of krum_geom, blocks_of, and the head of launch_pairdist_t
constexpr int kKrumLdsFloats = 8704;
constexpr int kKrumRowPad = 4;
constexpr int64_t kKrumMaxBlocks = 1024;
int krum_E(int D) {
    const int B = (D + 3) / 4;
    int E = 2048;
    while (4 * B * (E + kKrumRowPad) > kKrumLdsFloats) E >>= 1;
    return E;
}
int64_t krum_blocks_of(int64_t tiles, const Tuning& tu) {
    int64_t cap = kKrumMaxBlocks;
    if (tu.max_blocks > 0) cap = std::min<int64_t>(cap, tu.max_blocks);
    return std::max<int64_t>(1, std::min(tiles, cap));
}
struct KrumGrid {
    int64_t vec_blocks, elem_blocks, np;
};
KrumGrid krum_grid(int gm_E, int V, const Split& sp, const Tuning& tu) {
    int64_t vec_blocks = 0, elem_blocks = 0;
    if (sp.vec && sp.nvec > 0) {
        const int64_t EV = gm_E / V;
        vec_blocks = krum_blocks_of((sp.nvec + EV - 1) / EV, tu);
        elem_blocks = sp.edges() > 0 ? 1 : 0;
    } else {
        elem_blocks = krum_blocks_of((sp.n + gm_E - 1) / gm_E, tu);
    }
    const int64_t np = vec_blocks + elem_blocks;
    return KrumGrid{vec_blocks, elem_blocks, np};
}

constexpr uintptr_t kLeadBase = 0x7f0000100000, kOperandBase = 0x7e0000200000;  // 16-byte aligned, never read
const void* addr(uintptr_t a) { return reinterpret_cast<const void*>(a); }

// The split of n elements of size es led by an operand `phase` elements past a 16-byte boundary; !vec: a
// further input on another phase refuses the vector form.
Split make_split(size_t es, size_t phase, int64_t n, bool vec) {
    Split sp = fa::split_at(addr(kLeadBase + phase * es), es, (size_t)n);
    if (!vec) sp.require_input(addr(kOperandBase + (phase + 1) * es));
    return sp;
}

void pin(const char* what, const Split& sp, int64_t tile, int64_t cap, int max_blocks, int64_t vb, int64_t eb) {
    const fa::MeasureGrid g = fa::measure_grid(sp, tile, cap, max_blocks);
    check(g.vec_blocks == vb && g.elem_blocks == eb && g.np() == vb + eb, what, sp.V, tile, sp.n, max_blocks, sp.vec, 0);
}

}  // namespace

int main() {
    const int krum_D[3] = {3, 33, 128};
    check(krum_E(3) == 2048 && krum_E(33) == 128 && krum_E(128) == 64, "krum E", 0, 0, 0, 0, false, 0);
    for (size_t es : {(size_t)2, (size_t)4}) {
        const int V = (int)(16 / es);
        for (int stage = 0; stage < 4; ++stage) {  // 0: clip, 1..3: Krum at D = 3, 33, 128
            const int64_t tile = stage == 0 ? kClipTile : krum_E(krum_D[stage - 1]);
            const int64_t cap = stage == 0 ? kClipMaxBlocks : kKrumMaxBlocks;
            const int64_t ns[13] = {1, 3, tile - 1, tile, tile + 1, tile + V, 2 * tile - 1, 2 * tile + 5, tile * cap - 1,
                                    tile * cap, tile * cap + 1, tile * (cap + 3) + 7, 5 * tile * cap};
            for (size_t phase : {(size_t)0, (size_t)1})
                for (bool vec : {true, false})
                    for (int mb : {0, -1, 1, 7, (int)cap, (int)cap + 5})
                        for (int64_t n : ns) {
                            const Split sp = make_split(es, phase, n, vec);
                            const fa::MeasureGrid g = fa::measure_grid(sp, tile, cap, mb);
                            bool ok;
                            if (stage == 0) {
                                const ClipGrid l = clip_grid(sp, Tuning{mb});
                                ok = g.vec_blocks == l.vec_blocks && g.elem_blocks == l.elem_blocks &&
                                     g.np() == l.vec_blocks + l.elem_blocks;
                            } else {
                                const KrumGrid l = krum_grid((int)tile, V, sp, Tuning{mb});
                                ok = g.vec_blocks == l.vec_blocks && g.elem_blocks == l.elem_blocks && g.np() == l.np;
                            }
                            check(ok && sp.vec == vec, stage == 0 ? "clip" : "krum", V, tile, n, mb, vec, phase);
                        }
        }
    }
    // the numbers themselves: (vector workgroups, element workgroups)
    pin("below one tile", make_split(4, 0, 4095, true), 4096, 2048, 0, 1, 1);          // 1023 vectors, a tail of 3
    pin("one tile", make_split(4, 0, 4096, true), 4096, 2048, 0, 1, 0);
    pin("one tile and an edge", make_split(4, 0, 4097, true), 4096, 2048, 0, 1, 1);
    pin("two tiles", make_split(4, 0, 4100, true), 4096, 2048, 0, 2, 0);
    pin("above the cap", make_split(4, 0, (int64_t)4096 * 3000, true), 4096, 2048, 0, 2048, 0);
    pin("max_blocks below the cap", make_split(4, 0, (int64_t)4096 * 3000, true), 4096, 2048, 7, 7, 0);
    pin("mixed phases", make_split(4, 0, 10000, false), 4096, 2048, 0, 0, 3);
    pin("V = 8, a head", make_split(2, 1, 4096 + 7, true), 4096, 2048, 0, 1, 1);      // head 7, 512 vectors, no tail
    pin("krum D = 3", make_split(4, 0, 4099, true), 2048, 1024, 0, 2, 1);             // 1024 vectors, 512 a tile
    pin("krum D = 33", make_split(4, 0, 4099, true), 128, 1024, 0, 32, 1);            // 32 a tile
    pin("krum D = 128", make_split(2, 0, 100003, true), 64, 1024, 0, 1024, 1);        // 12500 vectors, 8 a tile
    std::printf("{\"checks\": %d, \"failed\": %d}\n", checks, failed);
    return failed ? 1 : 0;
}
