// fa_device.h -- device-side helpers shared by the kernel TUs: 16-byte loads, the store policies, the bf16 /
// fp16 conversions, the measure passes' fp64 sums and the element-type traits In<> / Out<>.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_internal.h"

namespace fa {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- helpers

template <bool NT>
__device__ __forceinline__ u32x4 ld16(const void* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    else return *reinterpret_cast<const u32x4*>(p);
}
// Store cache policies (fa_tuning.store_policy - 1): plain, nt, sc1 (write-through, the
// line is dropped from the XCD L2), sc0 sc1.  The asm stores need no waitcnt (nothing in
// the kernel reads the output back) but end with s_nop 1: hipcc does not pad hazards
// inside an asm statement and would otherwise overwrite the data VGPRs before the store
// has read them (cdna_hip_programming.md 5.7 item 1).
enum { kStPlain = 0, kStNt = 1, kStSc1 = 2, kStSc01 = 3 };
template <int SP>
__device__ __forceinline__ void st16(void* p, u32x4 v) {
    if constexpr (SP == kStNt) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
    else if constexpr (SP == kStSc1) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (SP == kStSc01)
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else *reinterpret_cast<u32x4*>(p) = v;
}
template <int SP>
__device__ __forceinline__ void st8(void* p, u32x2 v) {
    if constexpr (SP == kStNt) __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(p));
    else if constexpr (SP == kStSc1) asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (SP == kStSc01)
        asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else *reinterpret_cast<u32x2*>(p) = v;
}

__device__ __forceinline__ float bf16_to_f32(uint32_t h) { return __uint_as_float(h << 16); }

// Same integer rounding as oracle fa_oracle_f32_to_bf16 (NaN kept a quiet NaN).
__device__ __forceinline__ uint32_t f32_to_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// fp16 (FA_F16, IEEE binary16): plain casts on _Float16, which hipcc lowers to v_cvt_f32_f16 (exact,
// subnormals included) and v_cvt_f16_f32 (round-to-nearest-even under the kernels' default float mode, which
// keeps f16 and f32 denormals; beyond 65504 -> inf, NaN -> a quiet NaN).  bf16 buckets are tagged uint16_t,
// so fp16 takes _Float16 itself as its element tag.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ uint32_t f32_to_f16x2(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, f16x2{(_Float16)lo, (_Float16)hi});
}

// The measure passes (fa_clip.hip, fa_krum.hip).  acc + ((double)fl32(x - y))^2: the fp32 subtraction of the
// exactly widened inputs is one rounding, dd * dd is exact in fp64 (24 x 24 significand bits), so the fma's
// single rounding is that of the add.
__device__ __forceinline__ double sq_add(float x, float y, double acc) {
#pragma clang fp contract(off)
    const float d = x - y;
    const double dd = (double)d;
    return __builtin_fma(dd, dd, acc);
}
// The sum of v over the wave's 64 lanes, the same bits in every lane (each step adds the two halves of a pair,
// and fp64 addition commutes).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The workgroup half of a measure pass's reduction (fa_clip.hip, fa_geomed.hip): 256 lanes, one fp64 sum per
// (wave, row) in LDS, touched only by lane 0 of its wave between the two barriers.
constexpr int kMeasureThreads = 256, kMeasureWaves = kMeasureThreads / 64;
template <int ROWS>
struct MeasureLds {
    double acc[kMeasureWaves][ROWS];
};
template <int ROWS>
__device__ __forceinline__ void lds_zero(MeasureLds<ROWS>& l) {
    double* a = &l.acc[0][0];
    for (int i = threadIdx.x; i < kMeasureWaves * ROWS; i += kMeasureThreads) a[i] = 0.0;
    __syncthreads();
}
// partials[k * pstride + slot] = the workgroup's sum for row k < rows, the waves added in wave order.
template <int ROWS>
__device__ __forceinline__ void lds_flush(MeasureLds<ROWS>& l, int rows, double* partials, int64_t pstride, int64_t slot) {
    __syncthreads();
    for (int k = threadIdx.x; k < rows; k += kMeasureThreads) {
        double a = l.acc[0][k];
#pragma unroll
        for (int w = 1; w < kMeasureWaves; ++w) a += l.acc[w][k];
        partials[(int64_t)k * pstride + slot] = a;
    }
}

// Element-type traits: a lane owns 16 bytes of every input bucket.
template <typename T> struct In;
template <> struct In<float> {
    static constexpr int kVec = 4;
    __device__ static __forceinline__ void widen(u32x4 r, float* x) {
        x[0] = __uint_as_float(r.x); x[1] = __uint_as_float(r.y);
        x[2] = __uint_as_float(r.z); x[3] = __uint_as_float(r.w);
    }
    __device__ static __forceinline__ float scalar(const void* p, int64_t i) {
        return reinterpret_cast<const float*>(p)[i];
    }
};
template <> struct In<uint16_t> {
    static constexpr int kVec = 8;
    __device__ static __forceinline__ void widen(u32x4 r, float* x) {
        x[0] = __uint_as_float(r.x << 16); x[1] = __uint_as_float(r.x & 0xffff0000u);
        x[2] = __uint_as_float(r.y << 16); x[3] = __uint_as_float(r.y & 0xffff0000u);
        x[4] = __uint_as_float(r.z << 16); x[5] = __uint_as_float(r.z & 0xffff0000u);
        x[6] = __uint_as_float(r.w << 16); x[7] = __uint_as_float(r.w & 0xffff0000u);
    }
    __device__ static __forceinline__ float scalar(const void* p, int64_t i) {
        return bf16_to_f32(reinterpret_cast<const uint16_t*>(p)[i]);
    }
};
template <> struct In<_Float16> {
    static constexpr int kVec = 8;
    __device__ static __forceinline__ void widen(u32x4 r, float* x) {
        // the whole 16 bytes at once: __builtin_bit_cast of one element of r (r.y, ...) reads r's first dword
        const f16x8 h = __builtin_bit_cast(f16x8, r);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (float)h[j];
    }
    __device__ static __forceinline__ float scalar(const void* p, int64_t i) {
        return (float)reinterpret_cast<const _Float16*>(p)[i];
    }
};

template <typename T> struct Out;
template <> struct Out<float> {
    template <int V, int SP>
    __device__ static __forceinline__ void store(void* base, int64_t e, const float* a) {
        float* p = reinterpret_cast<float*>(base) + e;
#pragma unroll
        for (int j = 0; j < V; j += 4)
            st16<SP>(p + j, u32x4{__float_as_uint(a[j]), __float_as_uint(a[j + 1]), __float_as_uint(a[j + 2]),
                                  __float_as_uint(a[j + 3])});
    }
    __device__ static __forceinline__ void scalar(void* base, int64_t i, float a) {
        reinterpret_cast<float*>(base)[i] = a;
    }
};
// 16-bit outputs: pack2(lo, hi) is two elements rounded once each, in one dword (lo in the low half); the
// vector stores here and the packed LDS rows of the phased kernel (pack_rows16) are made of it.
template <typename T> struct Out16 {
    template <int V, int SP>
    __device__ static __forceinline__ void store(void* base, int64_t e, const float* a) {
        uint16_t* p = reinterpret_cast<uint16_t*>(base) + e;
        if constexpr (V == 8) {
            st16<SP>(p, u32x4{Out<T>::pack2(a[0], a[1]), Out<T>::pack2(a[2], a[3]), Out<T>::pack2(a[4], a[5]),
                              Out<T>::pack2(a[6], a[7])});
        } else {
            st8<SP>(p, u32x2{Out<T>::pack2(a[0], a[1]), Out<T>::pack2(a[2], a[3])});
        }
    }
};
template <> struct Out<uint16_t> : Out16<uint16_t> {
    __device__ static __forceinline__ uint32_t pack2(float lo, float hi) {
        return f32_to_bf16(lo) | (f32_to_bf16(hi) << 16);
    }
    __device__ static __forceinline__ void scalar(void* base, int64_t i, float a) {
        reinterpret_cast<uint16_t*>(base)[i] = (uint16_t)f32_to_bf16(a);
    }
};
template <> struct Out<_Float16> : Out16<_Float16> {
    __device__ static __forceinline__ uint32_t pack2(float lo, float hi) { return f32_to_f16x2(lo, hi); }
    __device__ static __forceinline__ void scalar(void* base, int64_t i, float a) {
        reinterpret_cast<_Float16*>(base)[i] = (_Float16)a;
    }
};

}  // namespace fa
