// fp8q_intq.h -- the uniform quantizers' scalar arithmetic shared by the forward (fp8q_int.hip) and the backward
// (fp8q_intgrad.hip): torch's min / max / clamp and the channel constants.  Internal linkage, as fp8q_common.h.
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

}  // namespace
