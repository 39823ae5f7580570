// fp8q_ocpq.h -- the device arithmetic of the hardware FP8 lane, shared by fp8q_ocp.hip (one scale per tensor or per output
// channel) and fp8q_ocp_block.hip (one scale per 1x128 / 128x1 / 128x128 tile): ONE copy of the NaN codes (OcpFmt), the scale
// of a range with its reciprocal (ocp_scale_pair), the division by reciprocal with its redo (code_exact, clamp_end, code4,
// code1) and decode (value_at, value4), and the stochastic-rounding codes of the fp8q_ocp*sr_* entries (code4_sr, code1_sr),
// whose draws and rounding are the MX lane's one copy in fp8q_mxq.h.  The contract these implement is stated in
// include/fp8q.h; the bound behind kOcpLo / kOcpHi is derived at the top of fp8q_ocp.hip.
// Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"
#include "fp8q_intq.h"
#include "fp8q_io.h"
#include "fp8q_mxq.h"       // MxSr, philox4x32, mx_draw8 / mx_draw4 / mx_draw1, mx_split4, mx_sr: the one copy of the draw and of SR

namespace {

// Fp8Fmt (fp8q_io.h: fmax, M, cvt4, value<B>) and the NaN codes, which decode does not leave to the instruction
template <int F>
struct OcpFmt;
template <>
struct OcpFmt<FP8Q_OCP_E4M3FN> : Fp8Fmt<FP8Q_OCP_E4M3FN> {
    static __device__ __forceinline__ bool is_nan(uint32_t code) { return (code & 0x7fu) == 0x7fu; }
};
template <>
struct OcpFmt<FP8Q_OCP_E5M2> : Fp8Fmt<FP8Q_OCP_E5M2> {
    static __device__ __forceinline__ bool is_nan(uint32_t code) { return (code & 0x7fu) > 0x7cu; }
};

constexpr float kOcpLo = 1.0f - 0x1p-21f, kOcpHi = 1.0f + 0x1p-21f;   // the interval around x * (1 / scale), see fp8q_ocp.hip

// {scale, 1/scale} of a range: scale = t_max(maxval, eps) / fmax; a reciprocal that overflows (scale below 2^-126) is stored
// as NaN, which sends every element under it to the division
template <int F>
__device__ __forceinline__ float4 ocp_scale_pair(float maxval, float eps)
{
    const float s = t_max(maxval, eps) / OcpFmt<F>::fmax;
    float r = 1.0f / s;
    if (fabsf(r) == __builtin_inff()) r = __builtin_nanf("");
    return make_float4(s, r, 0.0f, 0.0f);
}

// the contract's code of one element, by the IEEE division
template <int F>
__device__ __forceinline__ uint32_t code_exact(float v, float s)
{
    const float q = t_clamp(v / s, -OcpFmt<F>::fmax, OcpFmt<F>::fmax);
    return (q != q) ? 0x7fu : (OcpFmt<F>::cvt4(q, 0.0f, 0.0f, 0.0f) & 0xffu);
}

// a value's end of the interval, clamped (a NaN does not come out as one: its dword is redone)
template <int F>
__device__ __forceinline__ float clamp_end(float q, float m)
{
    return fminf(fmaxf(q * m, -OcpFmt<F>::fmax), OcpFmt<F>::fmax);
}

// the codes of four elements, k[j] = {scale, 1/scale} of element j's row (or tile)
template <int F>
__device__ __forceinline__ uint32_t code4(const float *v, const float4 *k)
{
    float lo[4], hi[4];
    bool nan = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float q0 = v[j] * k[j].y;
        nan |= q0 != q0;
        lo[j] = clamp_end<F>(q0, kOcpLo);
        hi[j] = clamp_end<F>(q0, kOcpHi);
    }
    uint32_t w = OcpFmt<F>::cvt4(lo[0], lo[1], lo[2], lo[3]);
    if (w != OcpFmt<F>::cvt4(hi[0], hi[1], hi[2], hi[3]) || nan) {
        w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= code_exact<F>(v[j], k[j].x) << (8 * j);
    }
    return w;
}

template <int F>
__device__ __forceinline__ uint32_t code1(float v, const float4 k)
{
    const float q0 = v * k.y;
    const uint32_t w = OcpFmt<F>::cvt4(clamp_end<F>(q0, kOcpLo), 0.0f, 0.0f, 0.0f) & 0xffu;
    if (w != (OcpFmt<F>::cvt4(clamp_end<F>(q0, kOcpHi), 0.0f, 0.0f, 0.0f) & 0xffu) || q0 != q0) return code_exact<F>(v, k.x);
    return w;
}

// ---- stochastic rounding: code = RNE(SR(q, r)) ----
// SR needs every bit of q = fl32(x / scale): f16, the 16 bits under the kept mantissa, moves by one with q's last bit, and a
// carry out of f16 + r flips a code.  The interval of code4 / code1 only says which code RNE gives, so the SR kernels take the
// IEEE division for EVERY element (the compiler's correctly rounded sequence: v_div_scale, v_rcp, the FMA corrections,
// v_div_fmas, v_div_fixup -- which is exact for a reciprocal that overflows or is subnormal, for quotients in fp32's subnormal
// range and for infinite and NaN scales, where a hand-written reciprocal-and-correction would have to prove it); 1 / scale is
// not read.  mx_sr<F> is the MX lane's rounding: FP8Q_OCP_E4M3FN / FP8Q_OCP_E5M2 are the ids of FP8Q_MX_E4M3FN / FP8Q_MX_E5M2
// (0 and 1), with the same M and bias.  Its result is on the grid, so the conversion instruction is exact on it; a NaN
// quotient is kept away from it and stores 0x7F.
static_assert(FP8Q_OCP_E4M3FN == FP8Q_MX_E4M3FN && FP8Q_OCP_E5M2 == FP8Q_MX_E5M2, "mx_sr<F> is indexed by the MX format ids");

// SR(q, r) of one element's quotient, a NaN as +0 with `nan` set
template <int F>
__device__ __forceinline__ float sr_q(float v, float s, uint32_t r, bool &nan)
{
    const float q = t_clamp(v / s, -OcpFmt<F>::fmax, OcpFmt<F>::fmax);
    nan = q != q;
    return nan ? 0.0f : mx_sr<F>(q, r);
}

// code4 under the 16-bit draws r[j] of the four elements
template <int F>
__device__ __forceinline__ uint32_t code4_sr(const float *v, const float4 *k, const uint32_t *r)
{
    float q[4];
    bool nan[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = sr_q<F>(v[j], k[j].x, r[j], nan[j]);
    uint32_t w = OcpFmt<F>::cvt4(q[0], q[1], q[2], q[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) w = nan[j] ? ((w & ~(0xffu << (8 * j))) | (0x7fu << (8 * j))) : w;
    return w;
}

template <int F>
__device__ __forceinline__ uint32_t code1_sr(float v, const float4 k, uint32_t r)
{
    bool nan;
    const float q = sr_q<F>(v, k.x, r, nan);
    return nan ? 0x7fu : (OcpFmt<F>::cvt4(q, 0.0f, 0.0f, 0.0f) & 0xffu);
}

// the draws of an aligned group of four flat indices i .. i + 3
__device__ __forceinline__ void sr_draws4(const MxSr &s, uint64_t i, uint32_t *r)
{
    uint32_t d[2];
    mx_draw4(s, i, d);
    mx_split4(d, r);
}

// code4_sr of the aligned group of four whose first flat index in x is e (offset + e a multiple of 4)
template <int F>
__device__ __forceinline__ uint32_t code4_sr_at(const MxSr &s, const float *v, const float4 *k, int64_t e)
{
    uint32_t r[4];
    sr_draws4(s, s.offset + (uint64_t)e, r);
    return code4_sr<F>(v, k, r);
}

// decode of byte B of a dword of codes: value * scale, a NaN code as the top of fp8q_ocp.hip has it
template <int F, int B>
__device__ __forceinline__ float value_at(uint32_t w, float s)
{
    const uint32_t code = (w >> (8 * B)) & 0xffu;
    const float y = OcpFmt<F>::template value<B>(w) * s;
    constexpr int M = OcpFmt<F>::M;
    const uint32_t nan = ((code & 0x80u) << 24) | 0x7fc00000u | ((code & ((1u << M) - 1u)) << (23 - M));
    return OcpFmt<F>::is_nan(code) ? __uint_as_float(nan) : y;
}

template <int F>
__device__ __forceinline__ void value4(uint32_t w, const float4 *k, float *y)
{
    y[0] = value_at<F, 0>(w, k[0].x);
    y[1] = value_at<F, 1>(w, k[1].x);
    y[2] = value_at<F, 2>(w, k[2].x);
    y[3] = value_at<F, 3>(w, k[3].x);
}

}  // namespace
