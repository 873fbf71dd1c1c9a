// fa_noise.hip -- the noise stage (fa.h "Noise stage") for CDNA4 (gfx950): a'_i = a_i + stddev * z_i, z_i the
// unit normal of element i of the bucket under (seed, stream, round).
//
// Per element the stage reads 4 bytes and writes 4 or 2.  The arithmetic is the other side of the ledger: one
// Philox4x32-10 call per four elements (20 32 x 32 -> 64 products, 20 xors of three words), and per word pair a
// logarithm (one division, a degree-4 Horner in s^2), a square root and a sine / cosine pair (two degree-4
// Horners), every step its own fp32 instruction.  No LDS; one cross-lane exchange where a lane's four elements
// straddle two Philox groups (below).
//
// Bit-exactness: as in fa_server_opt.hip nothing here may be fused: `#pragma clang fp contract(off)` at file
// scope and again in every function that does fp32 arithmetic (the flag travels with each instruction through
// inlining).  Division and square root are hipcc's correctly rounded forms, subnormals are kept.  The rule's
// functions are __host__ __device__: fa_noise_host (the audit entry, and the CPU suite's subject) runs the same
// source on the host, where the pragma keeps a host with FMA units from contracting as well.
//
// Two forms by fa::Split, as the other kernel TUs.  The vector form gives a lane the 16 bytes at elements
// head + 4 i .. + 3 of `avg`, that is elements g .. g + 3 of the bucket with g = idx0 + head + 4 i.  Philox
// group j makes the normals of elements 4 j .. 4 j + 3, so with PH = (idx0 + head) & 3 != 0 (a range shard or a
// piece that starts off a multiple of 4, or a pointer phase that does) every lane's vector takes 4 - PH normals
// of group j and PH of group j + 1.  Computing both per lane would double the stage's cost, so a wave walks a
// contiguous chunk of `iters` tiles of 64 vectors and lane l of tile t computes group J + 64 t + l alone: its
// upper neighbour's normals come by one __shfl per straddling element, and lane 63's from lane 0 of the next
// tile, which is computed one tile ahead.  A chunk costs iters + 1 group evaluations per lane instead of
// 2 iters; PH (wave-uniform, a template parameter, so that every register index is static) == 0 costs iters.
// The element form computes an element's whole group and keeps one normal: it runs on heads, tails and
// mixed 16-byte phases only.
//
// `out` may be `avg` itself for an f32 output: a lane reads its elements before it writes them, and no lane
// reads another's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

struct NoiseKey {
    uint32_t k0, k1;         // lo32(seed), hi32(seed)
    uint32_t round, stream;  // counter words 2 and 3
};

// fl() of the rule's constants (fa.h "Noise stage"), as hexadecimal literals: exact in any build.
constexpr float kSqrt2 = 0x1.6a09e6p+0f;  // fl(sqrt 2)
constexpr float kLn2 = 0x1.62e43p-1f;     // fl(ln 2)
constexpr float kPi4 = 0x1.921fb6p-1f;    // fl(pi / 4)
constexpr float kC3 = 0x1.555556p-2f, kC5 = 0x1.99999ap-3f, kC7 = 0x1.24924ap-3f, kC9 = 0x1.c71c72p-4f;     // fl(1/k)
constexpr float kS3 = -0x1.555556p-3f, kS5 = 0x1.111112p-7f, kS7 = -0x1.a01a02p-13f, kS9 = 0x1.71de3ap-19f;  // sine
constexpr float kK2 = -0x1p-1f, kK4 = 0x1.555556p-5f, kK6 = -0x1.6c16c2p-10f, kK8 = 0x1.a01a02p-16f;         // cosine

// Rule 1: Philox4x32-10 of counter (c0..c3) under key (k0, k1).  The 64-bit products are left to the compiler
// (v_mad_u64_u32 on gfx950: one instruction per product).
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                       uint32_t k1, uint32_t* r) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        c1 = (uint32_t)p1;
        c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0;
    r[1] = c1;
    r[2] = c2;
    r[3] = c3;
}

// Rule 2: R = sqrt(-2 ln u), u = (r + 1) 2^-32 with its top 24 bits kept.
__host__ __device__ __forceinline__ float noise_radius(uint32_t r) {
#pragma clang fp contract(off)
    const uint32_t N = r + 1u;  // 0 stands for 2^32
    uint32_t mant = 1u << 23;
    int e = 0;
    if (N != 0u) {
        const int lz = __builtin_clz(N);  // b = 31 - lz
        mant = (N << lz) >> 8;
        e = -1 - lz;
    }
    float m = (float)mant * 0x1p-23f;
    if (m > kSqrt2) {
        m = m * 0.5f;
        e = e + 1;
    }
    const float f = m - 1.0f;
    const float d = 2.0f + f;
    const float s = f / d;
    const float t = s * s;
    float p = kC9 * t;
    p = p + kC7;
    p = p * t;
    p = p + kC5;
    p = p * t;
    p = p + kC3;
    p = p * t;
    p = p * s;
    p = p + s;
    const float l = p + p;
    const float el = (float)e * kLn2;
    const float L = el + l;
    const float w = -2.0f * L;
    return __builtin_sqrtf(w);
}

// Rule 3: (cos, sin) of the angle q pi/2 + x, q the word's top two bits, x in [-pi/4, pi/4) from the next 24.
__host__ __device__ __forceinline__ void noise_direction(uint32_t r, float& co, float& si) {
#pragma clang fp contract(off)
    const uint32_t q = r >> 30;
    const int k = (int)((r & 0x3FFFFFFFu) >> 6);
    const float v = (float)(k - (1 << 23)) * 0x1p-23f;
    const float x = v * kPi4;
    const float y = x * x;
    float p = kS9 * y;
    p = p + kS7;
    p = p * y;
    p = p + kS5;
    p = p * y;
    p = p + kS3;
    p = p * y;
    p = p * x;
    const float sx = p + x;
    p = kK8 * y;
    p = p + kK6;
    p = p * y;
    p = p + kK4;
    p = p * y;
    p = p + kK2;
    p = p * y;
    const float cx = p + 1.0f;
    const float c = (q & 1u) ? sx : cx, s = (q & 1u) ? cx : sx;  // q: 0 (c, s), 1 (-s, c), 2 (-c, -s), 3 (s, -c)
    co = (q == 1u || q == 2u) ? -c : c;
    si = (q >= 2u) ? -s : s;
}

// Rules 1-4: the four unit normals of group j (elements 4 j .. 4 j + 3).
__host__ __device__ __forceinline__ void group_normals(const NoiseKey& key, uint64_t j, float* z) {
#pragma clang fp contract(off)
    uint32_t r[4];
    philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), key.round, key.stream, key.k0, key.k1, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float R = noise_radius(r[2 * h]);
        float c, s;
        noise_direction(r[2 * h + 1], c, s);
        z[2 * h] = R * c;
        z[2 * h + 1] = R * s;
    }
}

// Rule 4: a' = fl(a + fl(stddev z)).
__device__ __forceinline__ float noise_add(float a, float stddev, float z) {
#pragma clang fp contract(off)
    const float d = stddev * z;
    return a + d;
}

// Vector form.  Wave w of the grid walks chunks w, w + waves, ...; a chunk is `iters` tiles of 64 vectors, lane l
// of tile t owning vector i = (chunk iters + t) 64 + l: elements head + 4 i .. + 3 of avg and out, elements
// g0 + 4 i .. + 3 of the bucket (g0 = idx0 + head, PH = g0 & 3), whose first group is (g0 >> 2) + i.
template <typename OUT, int PH, int SP>
__global__ __launch_bounds__(256) void noise_vec_kernel(const NoiseKey key, const float stddev, const float* avg,
                                                        void* out, int64_t head, int64_t nvec, uint64_t g0, int iters,
                                                        int64_t nchunk) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t wpb = (int64_t)(blockDim.x >> 6);
    const int64_t waves = (int64_t)gridDim.x * wpb;
    const uint64_t j0 = g0 >> 2;
    for (int64_t c = (int64_t)blockIdx.x * wpb + (int64_t)(threadIdx.x >> 6); c < nchunk; c += waves) {
        const int64_t t0 = c * iters;  // the chunk's first tile
        float zc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (PH != 0) group_normals(key, j0 + (uint64_t)(t0 * 64 + lane), zc);
#pragma unroll 1
        for (int t = 0; t < iters; ++t) {
            const int64_t tile = (t0 + t) * 64;
            if (tile >= nvec) break;  // wave-uniform
            const int64_t i = tile + lane;
            float z[4];
            if constexpr (PH == 0) {
                if (i < nvec) group_normals(key, j0 + (uint64_t)i, z);
            } else {
                // the next tile's groups, one tile ahead: lane 63's upper neighbour is lane 0 of that tile
                float zn[4];
                group_normals(key, j0 + (uint64_t)(i + 64), zn);
                float up[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // [0, PH) used
#pragma unroll
                for (int k = 0; k < PH; ++k) up[k] = __shfl(lane == 0 ? zn[k] : zc[k], (lane + 1) & 63, 64);
#pragma unroll
                for (int k = 0; k < 4; ++k) z[k] = PH + k < 4 ? zc[(PH + k) & 3] : up[(PH + k) & 3];
#pragma unroll
                for (int k = 0; k < 4; ++k) zc[k] = zn[k];
            }
            if (i < nvec) {
                const int64_t e = head + i * 4;
                float a[4];
                In<float>::widen(ld16<true>(avg + e), a);
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = noise_add(a[k], stddev, z[k]);
                Out<OUT>::template store<4, SP>(out, e, a);
            }
        }
    }
}

// Element form over elements [0, head) and [tail0, n) (the whole array: head = tail0 = n), one per lane.
template <typename OUT>
__global__ __launch_bounds__(256) void noise_elem_kernel(const NoiseKey key, const float stddev, const float* avg,
                                                         void* out, int64_t head, int64_t tail0, int64_t n,
                                                         uint64_t idx0) {
    const int64_t cnt = head + (n - tail0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // one element per lane and trip: a 16-bit output (which cannot alias avg) would otherwise be vectorised
    // into four groups per lane, with SGPR spills
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cnt; s += stride) {
        const int64_t i = s < head ? s : tail0 + (s - head);
        const uint64_t g = idx0 + (uint64_t)i;
        float z[4];
        group_normals(key, g >> 2, z);
        const uint32_t ph = (uint32_t)g & 3u;
        const float zi = ph == 0u ? z[0] : ph == 1u ? z[1] : ph == 2u ? z[2] : z[3];
        Out<OUT>::scalar(out, i, noise_add(avg[i], stddev, zi));
    }
}

constexpr int64_t kElemMaxBlocks = 1 << 16;  // grid-stride beyond it
constexpr int kNoiseMaxIters = 8;            // tiles per chunk: a straddling launch costs 9/8 of an aligned one
constexpr int64_t kNoiseWaves = 256 * 16;    // chunks to aim for before a chunk grows: every SIMD of 256 CUs, 4 deep

int64_t blocks_for(int64_t work, int64_t per, const Tuning& tu, int64_t cap) {
    const int64_t g = (work + per - 1) / per;
    if (tu.max_blocks > 0) cap = std::min<int64_t>(cap, tu.max_blocks);
    return std::max<int64_t>(1, std::min(g, cap));
}

template <typename OUT, int PH>
hipError_t launch_noise_p(const NoiseKey& key, float stddev, const float* avg, void* out, uint64_t idx0, const Split& sp,
                          const Tuning& tu, hipStream_t s) {
    const int64_t tiles = (sp.nvec + 63) / 64;
    const int iters = (int)std::max<int64_t>(1, std::min<int64_t>(kNoiseMaxIters, tiles / kNoiseWaves));
    const int64_t nchunk = (tiles + iters - 1) / iters;
    hipLaunchKernelGGL((noise_vec_kernel<OUT, PH, kStSc1>),
                       dim3((unsigned)blocks_for(nchunk, tu.block / 64, tu, (int64_t)1 << 30)), dim3(tu.block), 0, s, key,
                       stddev, avg, out, sp.head, sp.nvec, idx0 + (uint64_t)sp.head, iters, nchunk);
    if (sp.edges() > 0)
        hipLaunchKernelGGL((noise_elem_kernel<OUT>), dim3(1), dim3(64), 0, s, key, stddev, avg, out, sp.head, sp.tail0(),
                           sp.n, idx0);
    return hipGetLastError();
}

template <typename OUT>
hipError_t launch_noise_t(const NoiseKey& key, float stddev, const float* avg, void* out, uint64_t idx0, const Split& sp,
                          const Tuning& tu, hipStream_t s) {
    if (sp.vec && sp.nvec > 0) {
        switch ((idx0 + (uint64_t)sp.head) & 3u) {
            case 0: return launch_noise_p<OUT, 0>(key, stddev, avg, out, idx0, sp, tu, s);
            case 1: return launch_noise_p<OUT, 1>(key, stddev, avg, out, idx0, sp, tu, s);
            case 2: return launch_noise_p<OUT, 2>(key, stddev, avg, out, idx0, sp, tu, s);
            default: return launch_noise_p<OUT, 3>(key, stddev, avg, out, idx0, sp, tu, s);
        }
    }
    hipLaunchKernelGGL((noise_elem_kernel<OUT>), dim3((unsigned)blocks_for(sp.n, tu.block, tu, kElemMaxBlocks)),
                       dim3(tu.block), 0, s, key, stddev, avg, out, sp.n, sp.n, sp.n, idx0);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_noise(const float* avg, void* out, fa_dtype odt, float stddev, uint64_t seed, uint32_t stream,
                        uint32_t round, uint64_t idx0, const Split& sp, const Tuning& tu, hipStream_t s) {
    if (sp.n <= 0) return hipSuccess;
    if (!sp.valid() || sp.V != 4 || !avg || !out || tu.block < 64 || tu.block % 64) return hipErrorInvalidValue;
    const NoiseKey key{(uint32_t)seed, (uint32_t)(seed >> 32), round, stream};
    switch (odt) {
        case FA_F32: return launch_noise_t<float>(key, stddev, avg, out, idx0, sp, tu, s);
        case FA_BF16: return launch_noise_t<uint16_t>(key, stddev, avg, out, idx0, sp, tu, s);
        case FA_F16: return launch_noise_t<_Float16>(key, stddev, avg, out, idx0, sp, tu, s);
    }
    return hipErrorInvalidValue;
}

void noise_host(uint64_t seed, uint32_t stream, uint32_t round, uint64_t idx0, size_t n, float* z) {
    const NoiseKey key{(uint32_t)seed, (uint32_t)(seed >> 32), round, stream};
    size_t done = 0;
    while (done < n) {
        const uint64_t g = idx0 + done;
        float zz[4];
        group_normals(key, g >> 2, zz);
        for (uint32_t k = (uint32_t)g & 3u; k < 4 && done < n; ++k) z[done++] = zz[k];
    }
}

}  // namespace fa
