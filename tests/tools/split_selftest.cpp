// split_selftest.cpp -- CPU test of the vector / element split of a launch (csrc/fa_split.h).
//
// fa::Split replaced four hand-written copies of one rule in the library's host code.  This program keeps those
// copies, verbatim, as the legacy_* functions below and compares the type with them exhaustively: both input
// element sizes, every 16-byte phase of the lead operand, every n in 0 .. 3V + 1 (so: no vector, a clamped head,
// one to three vectors, with and without a tail), and for every further operand both element sizes at every
// offset in 0 .. 31 from a 16-byte boundary.  Addresses are made from integers and never dereferenced.
// tests/test_host_sanitizers.py computes the number of checks from the same ranges.  Last line: one JSON
// line; exit code 1 if any check failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "fa_split.h"

namespace {

int checks = 0, failed = 0;
void check(bool ok, const char* what, size_t si, size_t phase, size_t n, size_t es, size_t off) {
    ++checks;
    if (ok) return;
    ++failed;
    if (failed <= 20)
        std::fprintf(stderr, "FAIL %s: si %zu phase %zu n %zu es %zu off %zu\n", what, si, phase, n, es, off);
}

const void* addr(uintptr_t a) { return reinterpret_cast<const void*>(a); }

// ---- the four spellings as they stood in reduce_on, sync_on, opt_on and clip_sumsq_on
struct Legacy {
    size_t phase;
    int64_t head, nvec;
};
Legacy legacy_split(const void* lead, size_t si, size_t n) {
    const int V = (int)(16 / si);
    const size_t phase = ((uintptr_t)lead % 16) / si;
    int64_t head = (int64_t)((V - phase) % V);
    if ((size_t)head > n) head = (int64_t)n;
    const int64_t nvec = (int64_t)(n - (size_t)head) / V;
    return Legacy{phase, head, nvec};
}
bool legacy_valid(int64_t head, int64_t nvec, int64_t V, int64_t n) {
    return !(head < 0 || nvec < 0 || head + nvec * V > n);
}
// a further input: the same 16-byte phase
bool legacy_input(const void* p, size_t si, size_t phase) { return ((uintptr_t)p % 16) / si == phase; }
// reduce_on's output
bool legacy_output(const void* dst, int64_t head, int V, size_t so) {
    const size_t out_vec_bytes = (size_t)V * so;  // 16 or 32 (f32 out of 16-bit) or 8 (16-bit out of f32)
    return ((uintptr_t)dst + (size_t)head * so) % std::min<size_t>(16, out_vec_bytes) == 0;
}
// init, the clip reference, the multi-pass fp32 scratch
bool legacy_f32(const void* p, int64_t head) { return ((uintptr_t)p + (size_t)head * 4) % 16 == 0; }
// opt_on's output (4 elements per vector)
bool legacy_opt_output(const void* out, int64_t head, size_t dsize) {
    return ((uintptr_t)out + (size_t)head * dsize) % (4 * dsize) == 0;
}

constexpr uintptr_t kLeadBase = 0x7f0000100000, kOperandBase = 0x7e0000200000;  // 16-byte aligned, never read

}  // namespace

int main() {
    for (size_t si : {(size_t)2, (size_t)4}) {
        const int V = (int)(16 / si);
        for (size_t phase = 0; phase < (size_t)V; ++phase) {
            const void* lead = addr(kLeadBase + phase * si);
            for (size_t n = 0; n <= (size_t)(3 * V + 1); ++n) {
                const fa::Split sp = fa::split_at(lead, si, n);
                const Legacy lg = legacy_split(lead, si, n);
                check(sp.head == lg.head && sp.V == V && sp.n == (int64_t)n && sp.vec, "head", si, phase, n, 0, 0);
                check(sp.nvec == lg.nvec, "nvec", si, phase, n, 0, 0);
                check(sp.valid() && legacy_valid(lg.head, lg.nvec, V, (int64_t)n), "valid", si, phase, n, 0, 0);
                // the refusals of the two hand-written checks: a negative head, negative vectors, vectors past n
                for (int bad = 0; bad < 3; ++bad) {
                    fa::Split b = sp;
                    if (bad == 0) b.head = -1;
                    if (bad == 1) b.nvec = -1;
                    if (bad == 2) b.nvec = lg.nvec + 1;
                    const bool lv = legacy_valid(b.head, b.nvec, V, (int64_t)n);
                    check(!b.valid() && !lv, "invalid", si, phase, n, 0, (size_t)bad);
                }
                {  // fa_trimmed.hip
                    const int64_t head = lg.head, nvec = lg.nvec;
                    const int64_t tail0 = head + nvec * V, edges = head + ((int64_t)n - tail0);
                    check(sp.tail0() == tail0, "tail0 (trimmed)", si, phase, n, 0, 0);
                    check(sp.edges() == edges, "edges (trimmed)", si, phase, n, 0, 0);
                }
                {  // fa_clip.hip
                    const int64_t head = lg.head, nvec = lg.nvec;
                    const int64_t edges = head + ((int64_t)n - (head + nvec * V));
                    check(sp.edges() == edges, "edges (clip)", si, phase, n, 0, 0);
                }
                if (V == 4) {  // fa_server_opt.hip
                    const int64_t head = lg.head, nvec = lg.nvec;
                    const int64_t tail0 = head + nvec * 4, edges = head + ((int64_t)n - tail0);
                    check(sp.tail0() == tail0, "tail0 (opt)", si, phase, n, 0, 0);
                    check(sp.edges() == edges, "edges (opt)", si, phase, n, 0, 0);
                }
                {  // a refused operand stays refused
                    fa::Split a = sp;
                    a.require_input(addr(kOperandBase + ((phase + 1) % (size_t)V) * si));
                    a.require_input(lead);
                    check(!a.vec, "sticky", si, phase, n, 0, 0);
                }
                for (size_t es : {(size_t)2, (size_t)4})
                    for (size_t off = 0; off < 32; off += es) {
                        const void* q = addr(kOperandBase + off);
                        fa::Split r = sp;
                        r.require(q, es);
                        if (es == si) {
                            fa::Split in = sp;
                            in.require_input(q);
                            check(in.vec == legacy_input(q, si, lg.phase), "input", si, phase, n, es, off);
                            // one rule: where the head is not clamped, an input is judged as any other operand
                            if ((int64_t)n >= sp.lead) check(in.vec == r.vec, "one rule", si, phase, n, es, off);
                        }
                        check(r.vec == legacy_output(q, lg.head, V, es), "output", si, phase, n, es, off);
                        if (es == 4) check(r.vec == legacy_f32(q, lg.head), "init/ref/scratch", si, phase, n, es, off);
                        if (V == 4)
                            check(r.vec == legacy_opt_output(q, lg.head, es), "opt output", si, phase, n, es, off);
                    }
            }
        }
    }
    std::printf("{\"checks\": %d, \"failed\": %d}\n", checks, failed);
    return failed ? 1 : 0;
}
