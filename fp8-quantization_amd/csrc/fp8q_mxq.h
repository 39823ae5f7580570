// fp8q_mxq.h -- the device arithmetic of the microscaling (MX) lane, shared by fp8q_mx.hip (blocks along the last dimension)
// and fp8q_mx_t.hip (blocks along dim 0): ONE copy of the block size, the formats' constants (MxFmt), the scale byte
// (scale_code / scale_inv / scale_value), the element conversions (mx_q, fp4_*, fp6_*, mx_code4 / mx_value4) and the integer
// maxima (umax4, umax_xor).  The contract these implement is stated once, in include/fp8q.h and in fp8q_mx.hip's header.
// Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"
#include "fp8q_io.h"

namespace {

constexpr int kMxBlock = 32;          // elements under one scale byte

// the FP8 formats: Fp8Fmt (fp8q_io.h: fmax, cvt4, value<B>) and what the scale byte needs; E2M1 converts in integer code below
template <int F>
struct MxFmt;
template <>
struct MxFmt<FP8Q_MX_E4M3FN> : Fp8Fmt<FP8Q_MX_E4M3FN> {
    static constexpr int emax = 8;
    static constexpr uint32_t man_fmax = 0x600000u;
};
template <>
struct MxFmt<FP8Q_MX_E5M2> : Fp8Fmt<FP8Q_MX_E5M2> {
    static constexpr int emax = 15;
    static constexpr uint32_t man_fmax = 0x600000u;
};
template <>
struct MxFmt<FP8Q_MX_E2M1> {
    static constexpr int emax = 2;
    static constexpr float fmax = 6.0f;
    static constexpr uint32_t man_fmax = 0x400000u;
};
// the 6-bit formats: M mantissa bits under 5 - M exponent bits of bias 2^(4 - M) - 1
template <>
struct MxFmt<FP8Q_MX_E2M3> {
    static constexpr int emax = 2;
    static constexpr float fmax = 7.5f;
    static constexpr uint32_t man_fmax = 0x700000u;
    static constexpr int M = 3, bias = 1;
};
template <>
struct MxFmt<FP8Q_MX_E3M2> {
    static constexpr int emax = 4;
    static constexpr float fmax = 28.0f;
    static constexpr uint32_t man_fmax = 0x600000u;
    static constexpr int M = 2, bias = 3;
};
template <int F>
constexpr bool kFp6 = F == FP8Q_MX_E2M3 || F == FP8Q_MX_E3M2;

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// the scale byte of a block whose largest |x| has the bits m
template <int F>
__device__ __forceinline__ uint32_t scale_code(uint32_t m, int ceil_rule)
{
    const int E = (int)(m >> 23);
    const int bump = (ceil_rule && (m & 0x7fffffu) > MxFmt<F>::man_fmax) ? 1 : 0;
    const int c = E - MxFmt<F>::emax + bump;
    return E == 255 ? 0xffu : (uint32_t)(c < 0 ? 0 : c);
}

// 2^(127 - code), the factor of the encoding side; code <= 253 here (E <= 254, emax >= 2), so the field is never 0
__device__ __forceinline__ float scale_inv(uint32_t code) { return __uint_as_float((254u - code) << 23); }

// X = 2^(code - 127)
__device__ __forceinline__ float scale_value(uint32_t code)
{
    return __uint_as_float(code == 0u ? 0x00400000u : (code == 0xffu ? 0x7fc00000u : code << 23));
}

template <int F>
__device__ __forceinline__ float mx_q(float v, float inv)
{
    return fminf(fmaxf(v * inv, -MxFmt<F>::fmax), MxFmt<F>::fmax);
}

// E2M1 code of a finite q within +-6: the midpoints below |q|, a tie to the even code, the sign in bit 3
__device__ __forceinline__ uint32_t fp4_code(float q)
{
    const float a = fabsf(q);
    const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                       (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
    return c | ((__float_as_uint(q) >> 28) & 8u);
}

// the value of an E2M1 code
__device__ __forceinline__ float fp4_value(uint32_t code)
{
    const uint32_t e = (code >> 1) & 3u, m = code & 1u;
    const uint32_t mag = e == 0u ? (m ? 0x3f000000u : 0u) : (((e + 126u) << 23) | (m << 22));
    return __uint_as_float(mag | ((code & 8u) << 28));
}

// FP6 code (M mantissa bits, exponent bias BIAS) of a finite q within +-fmax, the sign in bit 5.  A normal q: the exponent
// field rebiased, the 23 - M dropped mantissa bits rounded to nearest even on the integer, the carry running into the exponent
// (fmax itself is exact, so nothing passes code 31).  A subnormal q: |q| + 2^(24 - BIAS - M), whose unit in the last place is
// the grid's step 2^(1 - BIAS - M) -- the one fp32 addition rounds to nearest even and leaves m = 0 .. 2^M in the low bits,
// 2^M being the code of the smallest normal.
template <int M, int BIAS>
__device__ __forceinline__ uint32_t fp6_code(float q)
{
    constexpr int sh = 23 - M;
    constexpr uint32_t one = (uint32_t)(128 - BIAS) << 23;              // bits of 2^(1 - BIAS), the smallest normal
    constexpr uint32_t magic = (uint32_t)(127 + 24 - BIAS - M) << 23;
    const uint32_t a = abs_bits(q);
    const uint32_t t = a - ((uint32_t)(127 - BIAS) << 23);
    const uint32_t n = (t + ((1u << (sh - 1)) - 1u) + ((t >> sh) & 1u)) >> sh;
    const uint32_t s = __float_as_uint(__uint_as_float(a) + __uint_as_float(magic)) - magic;
    return (a >= one ? n : s) | ((__float_as_uint(q) >> 26) & 0x20u);
}

// the value of an FP6 code: its magnitude bits as an fp32's exponent and top mantissa bits -- a subnormal fp32 where e == 0 --
// times 2^(127 - BIAS), which is exact
template <int M, int BIAS>
__device__ __forceinline__ float fp6_value(uint32_t code)
{
    const uint32_t b = ((code & 0x1fu) << (23 - M)) | ((code & 0x20u) << 26);
    return __uint_as_float(b) * __uint_as_float((uint32_t)(254 - BIAS) << 23);
}

// The codes of four elements under the scale byte sc: FP8 a dword, FP6 the low 24 bits (element 0 in the low six), FP4 the low
// 16 bits (element 0 in the low nibble)
template <int F>
__device__ __forceinline__ uint32_t mx_code4(const float *v, uint32_t sc)
{
    if (sc == 0xffu) return (F == FP8Q_MX_E2M1 || kFp6<F>) ? 0u : 0x7f7f7f7fu;
    const float inv = scale_inv(sc);
    const float q0 = mx_q<F>(v[0], inv), q1 = mx_q<F>(v[1], inv), q2 = mx_q<F>(v[2], inv), q3 = mx_q<F>(v[3], inv);
    if constexpr (F == FP8Q_MX_E2M1) {
        return fp4_code(q0) | (fp4_code(q1) << 4) | (fp4_code(q2) << 8) | (fp4_code(q3) << 12);
    } else if constexpr (kFp6<F>) {
        constexpr int M = MxFmt<F>::M, B = MxFmt<F>::bias;
        return fp6_code<M, B>(q0) | (fp6_code<M, B>(q1) << 6) | (fp6_code<M, B>(q2) << 12) | (fp6_code<M, B>(q3) << 18);
    } else {
        return MxFmt<F>::cvt4(q0, q1, q2, q3);
    }
}

// value(elem) * X of element B of mx_code4()'s word; a NaN (a NaN code, a NaN scale) is the one quiet NaN
template <int F, int B>
__device__ __forceinline__ float mx_value_at(uint32_t w, float X)
{
    float v;
    if constexpr (F == FP8Q_MX_E2M1) v = fp4_value((w >> (4 * B)) & 0xfu);
    else if constexpr (kFp6<F>) v = fp6_value<MxFmt<F>::M, MxFmt<F>::bias>(w >> (6 * B));
    else v = MxFmt<F>::template value<B>(w);
    const float y = v * X;
    return (y != y) ? __uint_as_float(0x7fc00000u) : y;
}

template <int F>
__device__ __forceinline__ void mx_value4(uint32_t w, uint32_t sc, float *y)
{
    const float X = scale_value(sc);
    y[0] = mx_value_at<F, 0>(w, X);
    y[1] = mx_value_at<F, 1>(w, X);
    y[2] = mx_value_at<F, 2>(w, X);
    y[3] = mx_value_at<F, 3>(w, X);
}

__device__ __forceinline__ uint32_t umax4(const float *v)
{
    const uint32_t a = abs_bits(v[0]), b = abs_bits(v[1]), c = abs_bits(v[2]), d = abs_bits(v[3]);
    const uint32_t ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// max with the lane STEP away by xor, as one DPP move (every lane of the wave is live where this runs): quad_perm [1,0,3,2]
// and [2,3,0,1] for 1 and 2; for 4, once a quad agrees, row_half_mirror (lane i <-> 7 - i of its 8) reaches the other quad
template <int STEP>
__device__ __forceinline__ uint32_t umax_xor(uint32_t m)
{
    constexpr int ctrl = STEP == 1 ? 0xB1 : (STEP == 2 ? 0x4E : 0x141);
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, ctrl, 0xf, 0xf, false);
    return o > m ? o : m;
}

}  // namespace
