// fa_mx8_enc.hip -- MX8 replies (fa.h "MX8 replies") for CDNA4 (gfx950): the new model y against the model `sent`
// that the owners hold, as int8 codes q with one power-of-two scale e per 32 bucket elements, and the model
// g' = sent + decode(q, e) the owners will hold after it, in one fused element-wise pass.
//
// Per element the kernel reads y and sent (8 bytes for f32) and writes q, 1/32 byte of e, and g' once or twice (into
// the part's output and into `sent`): 9 + 1/32 bytes for f32.  The arithmetic is one fp32 subtract, an unsigned
// maximum on the bits, and per element one fp64 multiply and round (exact scaling: 2^(133 - E) is an fp64 value for
// every E, which it is not in fp32), the decoder's multiply and the decoder's add.  No LDS, no atomics, no inline
// assembly; the lanes of a block meet through cross-lane moves.
//
// Bit-exactness: `#pragma clang fp contract(off)` at file scope and in every function with fp32 arithmetic, as in
// fa_mx8.hip.  E comes from the maximum's bit pattern (mx8_scale_of_max, fa_mx8.h), never through frexp.  The block
// of an element is its bucket index >> 5: launches over [idx0, idx0 + n) with any idx0 give the bytes of one launch
// over the whole bucket, except in a block that a launch sees only part of -- there the caller runs the scales-only
// mode on the parts, takes the byte maximum and runs the scales-given mode (fa.h "MX8 replies", rule 6).
//
// Two forms.  The vector form takes whole blocks only: a lane owns 16 elements whose bucket index is a multiple of 16
// (y and sent in 16-byte loads, the 16 codes in one 16-byte store), two neighbouring lanes own a block and exchange
// their maxima once.  A launch whose pointers, after the head that ends at the first block boundary, are not all on a
// 16-byte boundary goes to the element form as a whole: a lane whose 16 elements straddled two blocks would need the
// maxima of three lanes, and such launches (odd pointer phases, a range that starts off a multiple of 16 elements
// from where its buffers are aligned) are not the ones that carry the bytes.  The element form gives a block 32
// consecutive lanes, one element each, the lanes outside the launch's range idle, and a five-step butterfly over the
// 32 lanes; it takes the head before the first block boundary and the tail after the last whole block (at most one
// block each, in one launch of one wave), launches without a vector part, and both scale modes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"
#include "fa_mx8.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

enum { kFused = 0, kScalesOnly = 1, kScalesGiven = 2 };

__device__ __forceinline__ float mx8_sub(float y, float s) {
#pragma clang fp contract(off)
    return y - s;
}
__device__ __forceinline__ uint32_t abs_bits(float d) { return __float_as_uint(d) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// Vector form: lane t owns vector t, elements head + 16 t .. + 15; bucket element idx0 + head is a multiple of 32 and
// nvec is even, so lanes t and t ^ 1 own one block and leave the loop together.  b0: the block e[0] scales.
template <typename T>
__global__ __launch_bounds__(256) void mx8_enc_vec_kernel(const void* y, const void* sent, int8_t* q, uint8_t* e,
                                                          void* out, void* out2, int64_t head, int64_t nvec,
                                                          uint64_t eb0) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nvec; t += stride) {
        const int64_t el = head + t * 16;
        float d[16], s[16];
        load_ref16<T>(y, el, d);
        load_ref16<T>(sent, el, s);
        uint32_t mb = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            d[k] = mx8_sub(d[k], s[k]);
            mb = umax(mb, abs_bits(d[k]));
        }
        mb = umax(mb, (uint32_t)__shfl_xor((int)mb, 1));
        const uint32_t E = mx8_scale_of_max(mb);
        if (!(t & 1)) e[eb0 + (uint64_t)(t >> 1)] = (uint8_t)E;
        const float sc = mx8_scale(E);
        u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = mx8_code(d[k], E);
            w[k >> 2] |= ((uint32_t)c & 0xffu) << (8 * (k & 3));
            s[k] = mx8_add(s[k], mx8_delta(c, sc));
        }
        st16<kStPlain>(q + el, w);
        if (out) store16<T>(out, el, s);
        if (out2) store16<T>(out2, el, s);
    }
}

// Element form over elements [a0, b0) and [a1, b1) of the launch, one per lane.  A range gets the lanes of every block
// it touches, 32 per block, lane l of a block the element with bucket index = l (mod 32); L0 is the lane count of the
// first range, L the count of both (multiples of 32, so the lanes of a block leave the loop together).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void mx8_enc_elem_kernel(const void* y, const void* sent, int8_t* q, uint8_t* e,
                                                           void* out, void* out2, int64_t a0, int64_t b0, int64_t a1,
                                                           int64_t b1, int64_t L0, int64_t L, uint64_t idx0) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t eb = idx0 >> 5;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < L; t += stride) {
        const bool first = t < L0;
        const int64_t lo = first ? a0 : a1, hi = first ? b0 : b1, tt = first ? t : t - L0;
        // the range's first lane stands for the start of the block that holds element lo
        const int64_t i = lo - (int64_t)((idx0 + (uint64_t)lo) & 31u) + tt;
        const bool active = i >= lo && i < hi;
        const uint64_t blk = ((idx0 + (uint64_t)i) >> 5) - eb;  // idx0 + i >= 0 also where i < 0
        float yv = 0.0f, sv = 0.0f;
        if (active) {
            yv = In<T>::scalar(y, i);
            sv = In<T>::scalar(sent, i);
        }
        const float d = mx8_sub(yv, sv);
        uint32_t E;
        if constexpr (MODE == kScalesGiven) {
            E = e[blk];
        } else {
            uint32_t mb = active ? abs_bits(d) : 0u;
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) mb = umax(mb, (uint32_t)__shfl_xor((int)mb, m, 32));
            E = mx8_scale_of_max(mb);
            if ((tt & 31) == 0) e[blk] = (uint8_t)E;
        }
        if constexpr (MODE != kScalesOnly) {
            if (active) {
                const int c = mx8_code(d, E);
                q[i] = (int8_t)c;
                const float x = mx8_add(sv, mx8_delta(c, mx8_scale(E)));
                if (out) Out<T>::scalar(out, i, x);
                if (out2) Out<T>::scalar(out2, i, x);
            }
        }
    }
}

constexpr int kEncBlock = 256;
constexpr int64_t kEncMaxBlocks = 1 << 14;  // grid-stride beyond it: 2^22 lanes in one trip

unsigned enc_blocks(int64_t work) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + kEncBlock - 1) / kEncBlock, kEncMaxBlocks));
}

// Lanes of the element form over [a, b): 32 per block touched.
int64_t elem_lanes(uint64_t idx0, int64_t a, int64_t b) {
    if (b <= a) return 0;
    return (int64_t)((((idx0 + (uint64_t)b - 1u) >> 5) - ((idx0 + (uint64_t)a) >> 5) + 1u) * 32u);
}

template <typename T, int MODE>
void launch_elem(const void* y, const void* sent, int8_t* q, uint8_t* e, void* out, void* out2, int64_t a0, int64_t b0,
                 int64_t a1, int64_t b1, uint64_t idx0, bool one_wave, hipStream_t s) {
    const int64_t L0 = elem_lanes(idx0, a0, b0), L = L0 + elem_lanes(idx0, a1, b1);
    if (L == 0) return;
    hipLaunchKernelGGL((mx8_enc_elem_kernel<T, MODE>), dim3(one_wave ? 1 : enc_blocks(L)), dim3(one_wave ? 64 : kEncBlock),
                       0, s, y, sent, q, e, out, out2, a0, b0, a1, b1, L0, L, idx0);
}

template <typename T>
hipError_t launch_enc_t(const void* y, const void* sent, uint64_t idx0, int8_t* q, uint8_t* e, void* out, void* out2,
                        int mode, const Split& sp, hipStream_t s) {
    const int64_t n = sp.n;
    if (mode == kScalesOnly) {
        launch_elem<T, kScalesOnly>(y, sent, q, e, out, out2, 0, n, 0, 0, idx0, false, s);
    } else if (mode == kScalesGiven) {
        launch_elem<T, kScalesGiven>(y, sent, q, e, out, out2, 0, n, 0, 0, idx0, false, s);
    } else if (sp.vec && sp.nvec > 0) {
        hipLaunchKernelGGL((mx8_enc_vec_kernel<T>), dim3(enc_blocks(sp.nvec)), dim3(kEncBlock), 0, s, y, sent, q, e, out,
                           out2, sp.head, sp.nvec, ((idx0 + (uint64_t)sp.head) >> 5) - (idx0 >> 5));
        if (sp.edges() > 0)  // the head and the tail: at most one block each
            launch_elem<T, kFused>(y, sent, q, e, out, out2, 0, sp.head, sp.tail0(), n, idx0, true, s);
    } else {
        launch_elem<T, kFused>(y, sent, q, e, out, out2, 0, n, 0, 0, idx0, false, s);
    }
    return hipGetLastError();
}

}  // namespace

// The split of one encoding: the head ends at the first block boundary of the bucket, the vectors are the whole
// blocks after it (two per block), and every pointer has to be on a 16-byte boundary there.
Split mx8_enc_split(const void* y, const void* sent, fa_dtype dt, uint64_t idx0, size_t n, const void* q,
                    const void* out, const void* out2) {
    const int64_t lead = (int64_t)((32u - (idx0 & 31u)) & 31u);
    const int64_t head = std::min<int64_t>(lead, (int64_t)n);
    Split sp{head, ((int64_t)n - head) / 32 * 2, (int64_t)n, 16, lead, true};
    const size_t es = dt == FA_F32 ? 4 : 2;
    sp.require(q, 1);
    sp.require(y, es);
    sp.require(sent, es);
    if (out) sp.require(out, es);
    if (out2) sp.require(out2, es);
    return sp;
}

hipError_t launch_mx8_encode(const void* y, const void* sent, fa_dtype dt, uint64_t idx0, int64_t n, int8_t* q,
                             uint8_t* e, void* out, void* out2, int mode, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!y || !sent || !e || (mode != kScalesOnly && !q) || mode < kFused || mode > kScalesGiven)
        return hipErrorInvalidValue;
    if (mode == kScalesOnly) out = out2 = nullptr;
    const Split sp = mx8_enc_split(y, sent, dt, idx0, (size_t)n, q, out, out2);
    if (!sp.valid()) return hipErrorInvalidValue;
    switch (dt) {
        case FA_F32: return launch_enc_t<float>(y, sent, idx0, q, e, out, out2, mode, sp, s);
        case FA_BF16: return launch_enc_t<uint16_t>(y, sent, idx0, q, e, out, out2, mode, sp, s);
        case FA_F16: return launch_enc_t<_Float16>(y, sent, idx0, q, e, out, out2, mode, sp, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace fa
