// fa_server_opt.hip -- the server-optimizer stage (FedAvgM, FedAdagrad, FedAdam, FedYogi) for CDNA4 (gfx950).
//
// Per element the stage reads the round's fp32 aggregate and the fp32 state (x, m, v), takes one step of the
// rule of fa.h "Server optimizer" and writes the state back and x' in the part's out dtype.  It is a stream:
// 4 reads and 4 writes per element (3 and 3 for momentum, which never touches v), a few dozen VALU
// operations, no LDS, no cross-lane traffic.
//
// Bit-exactness: every operation of the rule is one IEEE fp32 operation, so nothing here may be fused.  hipcc
// contracts a * b + c into an FMA in device code by default; `#pragma clang fp contract(off)` below (file
// scope, and again at the head of opt_step, whose body is the only arithmetic of the TU) turns that off.  The
// flag travels with each instruction, so inlining opt_step into the kernels keeps it.  Division and square
// root are hipcc's correctly rounded forms (the default for HIP), fp32 subnormals are kept (the default float
// mode of the kernels).
//
// Two forms, as the other kernel TUs: the vector form (16-byte loads of the aggregate and the state, 16-byte
// stores of the state, a 16-byte or 8-byte store of the output) when every pointer shares one 16-byte phase,
// and the element form for the head, the tail and mixed phases.  `out` may be the aggregate's own buffer for
// an f32 output: a lane reads its elements before it writes them, and no lane reads another's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "fa_device.h"
#include "fa_internal.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

struct NoOut {};  // OUT tag of a launch that writes the state only

// One step of rule RULE on one element (fa.h "Server optimizer"); kOptBoot is the bootstrap of a part
// without a master: x' = a, m' = v' = +0.
template <int RULE>
__device__ __forceinline__ void opt_step(const OptHyper& h, float a, float& x, float& m, float& v) {
#pragma clang fp contract(off)
    if constexpr (RULE == kOptBoot) {
        x = a;
        m = 0.0f;
        v = 0.0f;
    } else if constexpr (RULE == FA_OPT_MOMENTUM) {
        const float d = a - x;
        const float bm = h.beta1 * m;
        m = bm + d;
        const float step = h.lr * m;
        x = x + step;
    } else {
        const float d = a - x;
        const float bm = h.beta1 * m;
        const float cd = h.c1 * d;
        m = bm + cd;
        const float q = d * d;
        if constexpr (RULE == FA_OPT_ADAGRAD) {
            v = v + q;
        } else if constexpr (RULE == FA_OPT_ADAM) {
            const float bv = h.beta2 * v;
            const float cq = h.c2 * q;
            v = bv + cq;
        } else {  // FA_OPT_YOGI: v' = v - c2 q sign(v - q)
            const float u = h.c2 * q;
            const float s = v - q;
            const float dn = v - u, up = v + u;
            float vn = __uint_as_float(0x7fc00000u);  // s is NaN
            vn = s == 0.0f ? v : vn;
            vn = s < 0.0f ? up : vn;
            vn = s > 0.0f ? dn : vn;
            v = vn;
        }
        const float num = h.lr * m;
        const float root = __builtin_sqrtf(v);
        const float den = root + h.tau;
        const float step = num / den;
        x = x + step;
    }
}

template <int RULE> constexpr bool kReadsM = RULE != kOptBoot;
template <int RULE> constexpr bool kReadsV = RULE == FA_OPT_ADAGRAD || RULE == FA_OPT_ADAM || RULE == FA_OPT_YOGI;
// whether v is written: the adaptive rules always, the bootstrap when the part has one (wave-uniform)
template <int RULE>
__device__ __forceinline__ bool writes_v(const float* v) {
    if constexpr (RULE == kOptBoot) return v != nullptr;
    else return kReadsV<RULE>;
}

// Vector form: lane-vector i covers elements head + 4 i .. + 3 of every array (16-byte aligned there; a
// 16-bit output 8-byte aligned).  nt loads, write-through stores: every byte is touched once per round.
template <int RULE, typename OUT, int SP>
__global__ __launch_bounds__(256) void server_opt_vec_kernel(const OptHyper h, const float* avg, float* x, float* m,
                                                             float* v, void* out, int64_t head, int64_t nvec) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        const int64_t e = head + i * 4;
        const u32x4 ra = ld16<true>(avg + e);
        u32x4 rx = {}, rm = {}, rv = {};
        if constexpr (kReadsM<RULE>) rx = ld16<true>(x + e);
        if constexpr (kReadsM<RULE>) rm = ld16<true>(m + e);
        if constexpr (kReadsV<RULE>) rv = ld16<true>(v + e);
        float a[4], xs[4], ms[4], vs[4];
        In<float>::widen(ra, a);
        In<float>::widen(rx, xs);
        In<float>::widen(rm, ms);
        In<float>::widen(rv, vs);
#pragma unroll
        for (int j = 0; j < 4; ++j) opt_step<RULE>(h, a[j], xs[j], ms[j], vs[j]);
        Out<float>::template store<4, SP>(x, e, xs);
        Out<float>::template store<4, SP>(m, e, ms);
        if (writes_v<RULE>(v)) Out<float>::template store<4, SP>(v, e, vs);
        if constexpr (!std::is_same<OUT, NoOut>::value) Out<OUT>::template store<4, SP>(out, e, xs);
    }
}

// Element form over elements [0, head) and [tail0, n) (the whole array: head = tail0 = n), one per lane.
template <int RULE, typename OUT>
__global__ __launch_bounds__(256) void server_opt_elem_kernel(const OptHyper h, const float* avg, float* x, float* m,
                                                              float* v, void* out, int64_t head, int64_t tail0,
                                                              int64_t n) {
    const int64_t cnt = head + (n - tail0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cnt; s += stride) {
        const int64_t i = s < head ? s : tail0 + (s - head);
        const float a = avg[i];
        float xs = 0.0f, ms = 0.0f, vs = 0.0f;
        if constexpr (kReadsM<RULE>) xs = x[i];
        if constexpr (kReadsM<RULE>) ms = m[i];
        if constexpr (kReadsV<RULE>) vs = v[i];
        opt_step<RULE>(h, a, xs, ms, vs);
        x[i] = xs;
        m[i] = ms;
        if (writes_v<RULE>(v)) v[i] = vs;
        if constexpr (!std::is_same<OUT, NoOut>::value) Out<OUT>::scalar(out, i, xs);
    }
}

constexpr int64_t kElemMaxBlocks = 1 << 16;  // grid-stride beyond it
int64_t blocks_for(int64_t work, const Tuning& tu, int64_t cap) {
    int64_t g = (work + tu.block - 1) / tu.block;
    if (tu.max_blocks > 0) cap = std::min<int64_t>(cap, tu.max_blocks);
    return std::max<int64_t>(1, std::min(g, cap));
}

template <int RULE, typename OUT>
hipError_t launch_opt_t(const OptHyper& h, const float* avg, float* x, float* m, float* v, void* out, const Split& sp,
                        const Tuning& tu, hipStream_t s) {
    if (sp.vec && sp.nvec > 0) {
        hipLaunchKernelGGL((server_opt_vec_kernel<RULE, OUT, kStSc1>),
                           dim3((unsigned)blocks_for(sp.nvec, tu, (int64_t)1 << 30)), dim3(tu.block), 0, s, h, avg, x,
                           m, v, out, sp.head, sp.nvec);
        if (sp.edges() > 0)
            hipLaunchKernelGGL((server_opt_elem_kernel<RULE, OUT>), dim3(1), dim3(64), 0, s, h, avg, x, m, v, out,
                               sp.head, sp.tail0(), sp.n);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((server_opt_elem_kernel<RULE, OUT>), dim3((unsigned)blocks_for(sp.n, tu, kElemMaxBlocks)),
                       dim3(tu.block), 0, s, h, avg, x, m, v, out, sp.n, sp.n, sp.n);
    return hipGetLastError();
}

template <int RULE>
hipError_t launch_opt_r(const OptHyper& h, const float* avg, float* x, float* m, float* v, void* out, fa_dtype odt,
                        const Split& sp, const Tuning& tu, hipStream_t s) {
    if (!out) return launch_opt_t<RULE, NoOut>(h, avg, x, m, v, out, sp, tu, s);
    switch (odt) {
        case FA_F32: return launch_opt_t<RULE, float>(h, avg, x, m, v, out, sp, tu, s);
        case FA_BF16: return launch_opt_t<RULE, uint16_t>(h, avg, x, m, v, out, sp, tu, s);
        case FA_F16: return launch_opt_t<RULE, _Float16>(h, avg, x, m, v, out, sp, tu, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_server_opt(int rule, const OptHyper& h, const float* avg, float* x, float* m, float* v, void* out,
                             fa_dtype odt, const Split& sp, const Tuning& tu, hipStream_t s) {
    if (sp.n <= 0) return hipSuccess;
    if (!sp.valid() || sp.V != 4 || !avg || !x || !m) return hipErrorInvalidValue;
    if (!v && (rule == FA_OPT_ADAGRAD || rule == FA_OPT_ADAM || rule == FA_OPT_YOGI)) return hipErrorInvalidValue;
#define FA_OPT_RULE(R) \
    case R: return launch_opt_r<R>(h, avg, x, m, v, out, odt, sp, tu, s)
    switch (rule) {
        FA_OPT_RULE(kOptBoot);
        FA_OPT_RULE(FA_OPT_MOMENTUM);
        FA_OPT_RULE(FA_OPT_ADAGRAD);
        FA_OPT_RULE(FA_OPT_ADAM);
        FA_OPT_RULE(FA_OPT_YOGI);
    }
#undef FA_OPT_RULE
    return hipErrorInvalidValue;
}

}  // namespace fa
