// fp8q_io.h -- what the code lanes share (fp8q_ocp.hip: per-tensor / per-channel OCP FP8; fp8q_mx.hip: block-scaled MX).
//   - the modes of a launch, kEncode / kDecode / kQuant;
//   - a lane's elements on either side: fp32, half (T = F16 / BF16 of fp8q_half.h), codes.  load16: 16 consecutive elements,
//     the 16-byte loads issued before anything reads them; load4 / store4: one group of 4; load1 / store1: the elementwise
//     routes.  A half store rounds the fp32 value once (narrow1 / narrow2);
//   - the hardware FP8 conversions, Fp8Fmt<F>: fmax, M, cvt4 (four values -> a dword of codes) and value<B> (byte B of a dword
//     -> its value), thin wrappers over the four conversion builtins.  OcpFmt / MxFmt derive from it and add what is theirs;
//   - the host side of a launch: value_side_misaligned() and io_dispatch(), the one (mode, in_type, out_type) -> <IN, OUT>
//     ladder.
// Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"
#include "fp8q_half.h"

namespace {

enum { kEncode, kDecode, kQuant };

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
        const u4v *q = reinterpret_cast<const u4v *>(p);
        const u4v a = ldv<NT>(q), b = ldv<NT>(q + 1);
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) T::widen2(w[j], v[2 * j], v[2 * j + 1]);
    }
    template <bool NT>
    static __device__ __forceinline__ void load4(const elem *p, float *v)
    {
        const u2v t = ldv<NT>(reinterpret_cast<const u2v *>(p));
        T::widen2(t.x, v[0], v[1]);
        T::widen2(t.y, v[2], v[3]);
    }
    template <bool NT>
    static __device__ __forceinline__ void store4(elem *p, const float *v)
    {
        stv<NT>(reinterpret_cast<u2v *>(p), u2v{T::narrow2(v[0], v[1]), T::narrow2(v[2], v[3])});
    }
    static __device__ __forceinline__ float load1(const elem *p) { return T::widen1(*p); }
    static __device__ __forceinline__ void store1(elem *p, float v) { *p = T::narrow1(v); }
};

struct IoCodes {
    typedef uint8_t elem;
    template <bool NT>
    static __device__ __forceinline__ uint32_t load4(const elem *p) { return ldv<NT>(reinterpret_cast<const uint32_t *>(p)); }
};

// ---- the hardware FP8 conversions: F is FP8Q_OCP_* and FP8Q_MX_* alike ----
static_assert(FP8Q_OCP_E4M3FN == FP8Q_MX_E4M3FN && FP8Q_OCP_E5M2 == FP8Q_MX_E5M2, "one tag per FP8 format for both lanes");

// cvt4: four values (finite, within +-fmax) -> four codes in a dword, the first in the low byte (RNE, subnormals, -0);
// value<B>: the value of byte B of a dword of codes
template <int F>
struct Fp8Fmt;
template <>
struct Fp8Fmt<FP8Q_OCP_E4M3FN> {
    static constexpr float fmax = 448.0f;
    static constexpr int M = 3;
    static __device__ __forceinline__ uint32_t cvt4(float a, float b, float c, float d)
    {
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
        return (uint32_t)w;
    }
    template <int B>
    static __device__ __forceinline__ float value(uint32_t w) { return __builtin_amdgcn_cvt_f32_fp8((int)w, B); }
};
template <>
struct Fp8Fmt<FP8Q_OCP_E5M2> {
    static constexpr float fmax = 57344.0f;
    static constexpr int M = 2;
    static __device__ __forceinline__ uint32_t cvt4(float a, float b, float c, float d)
    {
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, w, false);
        w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
        return (uint32_t)w;
    }
    template <int B>
    static __device__ __forceinline__ float value(uint32_t w) { return __builtin_amdgcn_cvt_f32_bf8((int)w, B); }
};

// ---- host side ----
// a value side (type = FP8Q_DT_*) off its element's alignment; type < 0: the side holds codes, which have none
inline bool value_side_misaligned(const void *p, int type)
{
    return type < 0 ? false : (((uintptr_t)p) & (uintptr_t)(type == FP8Q_DT_F32 ? 3 : 1)) != 0;
}

// f(IoF32{}) / f(IoH16<F16>{}) / f(IoH16<BF16>{}) for a value side of `type`
template <class Fn>
inline void value_io(int type, Fn &&f)
{
    if (type == FP8Q_DT_F32) f(IoF32{});
    else if (type == FP8Q_DT_F16) f(IoH16<F16>{});
    else f(IoH16<BF16>{});
}

// f(Const<MODE>{}, IN{}, OUT{}) for a launch of `mode` whose value side(s) are in_type / out_type (FP8Q_DT_*, -1 for the side
// that holds codes).  Eleven pairs: encode from and decode to each of the three value types; quantize fp32 -> fp32 and a half
// type -> fp32 or itself (check_types() of fp8q_half.h has refused every other pair).
template <class Fn>
inline void io_dispatch(int mode, int in_type, int out_type, Fn &&f)
{
    if (mode == kEncode) {
        value_io(in_type, [&](auto in) { f(Const<kEncode>{}, in, IoCodes{}); });
    } else if (mode == kDecode) {
        value_io(out_type, [&](auto out) { f(Const<kDecode>{}, IoCodes{}, out); });
    } else {
        value_io(in_type, [&](auto in) {
            if (out_type == FP8Q_DT_F32) f(Const<kQuant>{}, in, IoF32{});
            else f(Const<kQuant>{}, in, in);
        });
    }
}

}  // namespace
