// fp8q_half.h -- what the kernels on IEEE fp16 / bfloat16 tensors share (fp8q_h16.hip: the FP8 lane, fp8q_inth16.hip: the
// uniform INT lane, fp8q_codec_h16.hip: their storage codes, fp8q_io.h: the code lanes): the dword vectors every unit names
// its 8- and 16-byte words by (u2v, u4v, u4v2), the exact widening to fp32 (widen1 / widen2 / widen8), the single rounding
// back to the storage type (narrow1 / narrow2 / store_half8), the scalar a lane takes around a body of 16-byte groups
// (scalar_of), and the check of an (x_type, y_type) pair.  Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"

namespace {

typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef __bf16 b2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef uint32_t u4v2 __attribute__((ext_vector_type(4), aligned(2)));   // 16 bytes wherever a half element may start

struct F16 {
    static __device__ __forceinline__ void widen2(uint32_t w, float &a, float &b)
    {
        const h2v h = __builtin_bit_cast(h2v, w);
        a = (float)h.x;
        b = (float)h.y;
    }
    static __device__ __forceinline__ uint32_t narrow2(float a, float b)
    {
        asm volatile("" : "+v"(a), "+v"(b));   // (see narrow1)
        const f2v v = {a, b};
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, h2v));
    }
    static __device__ __forceinline__ float widen1(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
    static __device__ __forceinline__ uint16_t narrow1(float a)
    {
        // the fp32 result is a value of its own: without this the compiler folds the quantizer's last multiplication and
        // the conversion into v_fma_mixlo_f16, which rounds the exact product ONCE to fp16 -- not fl16(fl32(r * s))
        asm volatile("" : "+v"(a));
        return __builtin_bit_cast(uint16_t, (_Float16)a);
    }
};

struct BF16 {
    static __device__ __forceinline__ void widen2(uint32_t w, float &a, float &b)
    {
        a = __uint_as_float(w << 16);
        b = __uint_as_float(w & 0xffff0000u);
    }
    static __device__ __forceinline__ uint32_t narrow2(float a, float b)
    {
        const f2v v = {a, b};
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, b2v));
    }
    static __device__ __forceinline__ float widen1(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }
    static __device__ __forceinline__ uint16_t narrow1(float a) { return __builtin_bit_cast(uint16_t, (__bf16)a); }
};

// the 8 elements of a 16-byte word
template <class T>
__device__ __forceinline__ void widen8(const u4v w, float (&e)[8])
{
    T::widen2(w.x, e[0], e[1]);
    T::widen2(w.y, e[2], e[3]);
    T::widen2(w.z, e[4], e[5]);
    T::widen2(w.w, e[6], e[7]);
}

// 8 values, each rounded once to T, as 16 bytes at whatever 2-byte phase y has
template <class T, bool NT = false>
__device__ __forceinline__ void store_half8(uint16_t *y, const float *e)
{
    const u4v2 w = {T::narrow2(e[0], e[1]), T::narrow2(e[2], e[3]), T::narrow2(e[4], e[5]), T::narrow2(e[6], e[7])};
    if (NT)
        __builtin_nontemporal_store(w, reinterpret_cast<u4v2 *>(y));
    else
        *reinterpret_cast<u4v2 *>(y) = w;
}

// the element in front of a body of 16-byte groups (tid < head) or behind it (lanes 32 ..) that this lane takes, or -1
__device__ __forceinline__ int64_t scalar_of(int tid, int64_t head, int64_t tail0, int64_t n)
{
    if (tid < head) return tid;
    if (tid >= 32 && tail0 + (tid - 32) < n) return tail0 + (tid - 32);
    return -1;
}

template <class T, bool YF32>
__device__ __forceinline__ void store1(void *y, int64_t e, float v)
{
    if (YF32)
        reinterpret_cast<float *>(y)[e] = v;
    else
        reinterpret_cast<uint16_t *>(y)[e] = T::narrow1(v);
}

inline bool half_type(int t) { return t == FP8Q_DT_F16 || t == FP8Q_DT_BF16; }

inline int check_types(int x_type, int y_type)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    if (y_type != FP8Q_DT_F32 && y_type != x_type) return FP8Q_EINVAL;
    return FP8Q_OK;
}

}  // namespace
