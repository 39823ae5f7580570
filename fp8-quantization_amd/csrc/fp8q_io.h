// fp8q_io.h -- a lane's elements on either side of the code lanes (fp8q_ocp.hip: per-tensor / per-channel OCP FP8;
// fp8q_mx.hip: block-scaled MX): fp32, half (T = F16 / BF16 of fp8q_half.h), codes.  load16: 16 consecutive elements, the
// 16-byte loads issued before anything reads them; load4 / store4: one group of 4; load1 / store1: the elementwise routes.
// A half store rounds the fp32 value once (narrow1 / narrow2).  Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"
#include "fp8q_half.h"

namespace {

typedef uint32_t vu4 __attribute__((ext_vector_type(4)));
typedef uint32_t vu2 __attribute__((ext_vector_type(2)));

struct IoF32 {
    typedef float elem;
    template <bool NT>
    static __device__ __forceinline__ void load16(const elem *p, float *v)
    {
        const vf4 *q = reinterpret_cast<const vf4 *>(p);
        vf4 t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = ldv<NT>(q + j);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[4 * j] = t[j].x;
            v[4 * j + 1] = t[j].y;
            v[4 * j + 2] = t[j].z;
            v[4 * j + 3] = t[j].w;
        }
    }
    template <bool NT>
    static __device__ __forceinline__ void load4(const elem *p, float *v)
    {
        const vf4 t = ldv<NT>(reinterpret_cast<const vf4 *>(p));
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
    template <bool NT>
    static __device__ __forceinline__ void store4(elem *p, const float *v)
    {
        stv<NT>(reinterpret_cast<vf4 *>(p), vf4{v[0], v[1], v[2], v[3]});
    }
    static __device__ __forceinline__ float load1(const elem *p) { return *p; }
    static __device__ __forceinline__ void store1(elem *p, float v) { *p = v; }
};

template <class T>
struct IoH16 {
    typedef uint16_t elem;
    template <bool NT>
    static __device__ __forceinline__ void load16(const elem *p, float *v)
    {
        const vu4 *q = reinterpret_cast<const vu4 *>(p);
        const vu4 a = ldv<NT>(q), b = ldv<NT>(q + 1);
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) T::widen2(w[j], v[2 * j], v[2 * j + 1]);
    }
    template <bool NT>
    static __device__ __forceinline__ void load4(const elem *p, float *v)
    {
        const vu2 t = ldv<NT>(reinterpret_cast<const vu2 *>(p));
        T::widen2(t.x, v[0], v[1]);
        T::widen2(t.y, v[2], v[3]);
    }
    template <bool NT>
    static __device__ __forceinline__ void store4(elem *p, const float *v)
    {
        stv<NT>(reinterpret_cast<vu2 *>(p), vu2{T::narrow2(v[0], v[1]), T::narrow2(v[2], v[3])});
    }
    static __device__ __forceinline__ float load1(const elem *p) { return T::widen1(*p); }
    static __device__ __forceinline__ void store1(elem *p, float v) { *p = T::narrow1(v); }
};

struct IoCodes {
    typedef uint8_t elem;
    template <bool NT>
    static __device__ __forceinline__ uint32_t load4(const elem *p) { return ldv<NT>(reinterpret_cast<const uint32_t *>(p)); }
};

}  // namespace
