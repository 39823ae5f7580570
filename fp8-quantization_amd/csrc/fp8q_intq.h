// fp8q_intq.h -- the uniform quantizers' scalar arithmetic shared by the forward (fp8q_int.hip), the backward
// (fp8q_intgrad.hip) and the integer codes (fp8q_intcodec.hip): torch's min / max / clamp, the channel constants and the
// integer level of an element.  Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"

namespace {

__device__ __forceinline__ float t_min(float a, float b)   // torch.min(a, b) of the scalar loop: a unless b < a
{
    return (a != a) ? a : ((b != b) ? b : (b < a ? b : a));
}
__device__ __forceinline__ float t_max(float a, float b)
{
    return (a != a) ? a : ((b != b) ? b : (b > a ? b : a));
}
__device__ __forceinline__ float t_clamp(float v, float lo, float hi)   // torch.clamp: NaN passes, v when equal
{
    return (v != v) ? v : (v < lo ? lo : (v > hi ? hi : v));
}

// {scale, 1/scale, zp, -}
__device__ __forceinline__ float4 consts_of(float delta, float zf, bool symmetric, float lo, float hi, float eps)
{
    const float s = t_max(delta, eps);
    const float zp = symmetric ? 0.0f : t_clamp(rintf(zf), lo, hi);
    return make_float4(s, 1.0f / s, zp, 0.0f);
}

// t = clamp(rint(v / scale) + zp, lo, hi), k = consts_of(): the ONE definition of the rounding (the reciprocal-then-redo
// rule is derived at the top of fp8q_int.hip).  int_one() dequantizes it, fp8q_intcodec.hip stores it.
__device__ __forceinline__ float int_level(float v, const float4 k, float lo, float hi)
{
    const float q0 = v * k.y;
    float rq = rintf(q0);
    if (fabsf(q0 - rq) >= 0.5f - fabsf(q0) * 0x1p-20f) rq = rintf(v / k.x);
    return t_clamp(rq + k.z, lo, hi);
}

}  // namespace
