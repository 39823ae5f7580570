// fp8q_mxq.h -- the device arithmetic of the microscaling (MX) lane, shared by fp8q_mx.hip (blocks along the last dimension)
// and fp8q_mx_t.hip (blocks along dim 0): ONE copy of the block size, the formats' constants (MxFmt), the scale byte
// (scale_code / scale_inv / scale_value), the element conversions (mx_q, fp4_*, fp6_*, mx_pack4, mx_code4 / mx_value4), the
// stochastic rounding in front of them (philox4x32, mx_draw*, mx_sr, mx_code4_sr) and the integer maxima (umax4, umax_xor).
// The contract these implement is stated once, in include/fp8q.h and in fp8q_mx.hip's header.
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

// The codes of four clamped q: FP8 a dword, FP6 the low 24 bits (element 0 in the low six), FP4 the low 16 bits (element 0 in
// the low nibble)
template <int F>
__device__ __forceinline__ uint32_t mx_pack4(float q0, float q1, float q2, float q3)
{
    if constexpr (F == FP8Q_MX_E2M1) {
        return fp4_code(q0) | (fp4_code(q1) << 4) | (fp4_code(q2) << 8) | (fp4_code(q3) << 12);
    } else if constexpr (kFp6<F>) {
        constexpr int M = MxFmt<F>::M, B = MxFmt<F>::bias;
        return fp6_code<M, B>(q0) | (fp6_code<M, B>(q1) << 6) | (fp6_code<M, B>(q2) << 12) | (fp6_code<M, B>(q3) << 18);
    } else {
        return MxFmt<F>::cvt4(q0, q1, q2, q3);
    }
}

// The codes of four elements under the scale byte sc, packed as mx_pack4 packs them
template <int F>
__device__ __forceinline__ uint32_t mx_code4(const float *v, uint32_t sc)
{
    if (sc == 0xffu) return (F == FP8Q_MX_E2M1 || kFp6<F>) ? 0u : 0x7f7f7f7fu;
    const float inv = scale_inv(sc);
    const float q0 = mx_q<F>(v[0], inv), q1 = mx_q<F>(v[1], inv), q2 = mx_q<F>(v[2], inv), q3 = mx_q<F>(v[3], inv);
    return mx_pack4<F>(q0, q1, q2, q3);
}

// ---- stochastic rounding (the fp8q_mxsr_* entries; include/fp8q.h states the draw and the rounding) ----
// seed and offset of a call; the flat index of element e of x as it lies is offset + e mod 2^64
struct MxSr {
    uint32_t k0, k1;              // seed & 0xffffffff, seed >> 32
    uint64_t offset;              // a multiple of 8
};

inline MxSr mx_sr_args(uint64_t seed, uint64_t offset) { return MxSr{(uint32_t)seed, (uint32_t)(seed >> 32), offset}; }

// Philox4x32-10 (Salmon et al., SC'11), the standard constants; the key is bumped after every round (the last bump is unused)
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                           uint32_t *out)
{
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// the call of the eight elements i .. i + 7, i a multiple of 8: word j holds the draws of elements i + 2j (low half) and
// i + 2j + 1 (high half)
__device__ __forceinline__ void mx_draw8(const MxSr &s, uint64_t i, uint32_t *w)
{
    const uint64_t g = i >> 3;
    philox4x32((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, s.k0, s.k1, w);
}

// the two words of the aligned group of four i .. i + 3 (i a multiple of 4): words 0, 1 or 2, 3 of its call
__device__ __forceinline__ void mx_draw4(const MxSr &s, uint64_t i, uint32_t *w)
{
    uint32_t o[4];
    mx_draw8(s, i & ~(uint64_t)7, o);
    const bool hi = (i & 4u) != 0u;
    w[0] = hi ? o[2] : o[0];
    w[1] = hi ? o[3] : o[1];
}

// the 16 bits of element i alone (the general routes: a call per element, no rate is claimed there)
__device__ __forceinline__ uint32_t mx_draw1(const MxSr &s, uint64_t i)
{
    uint32_t w[2];
    mx_draw4(s, i & ~(uint64_t)3, w);
    const uint32_t v = (i & 2u) ? w[1] : w[0];
    return (v >> (16 * (uint32_t)(i & 1u))) & 0xffffu;
}

// the four draws of a group out of its two words
__device__ __forceinline__ void mx_split4(const uint32_t *w, uint32_t *r)
{
    r[0] = w[0] & 0xffffu;
    r[1] = w[0] >> 16;
    r[2] = w[1] & 0xffffu;
    r[3] = w[1] >> 16;
}

// mantissa bits and exponent bias of the element formats, for the rounding below
template <int F>
struct MxGrid {
    static constexpr int M = MxFmt<F>::M, bias = MxFmt<F>::bias;
};
template <>
struct MxGrid<FP8Q_MX_E4M3FN> {
    static constexpr int M = 3, bias = 7;
};
template <>
struct MxGrid<FP8Q_MX_E5M2> {
    static constexpr int M = 2, bias = 15;
};
template <>
struct MxGrid<FP8Q_MX_E2M1> {
    static constexpr int M = 1, bias = 1;
};

// SR(q, r): the fp32 on F's grid that q (finite, within +-fmax) rounds to under the 16-bit draw r -- one of its two
// neighbours, away from zero with probability floor(f * 2^16) / 2^16.  Normal range: the 16 bits under the kept mantissa plus
// r carry into it, the carry running into the exponent (fmax is a grid point, so nothing passes it).  Format-subnormal
// range: |q| in units of 2^-16 of the grid's step by ONE fp32 product (exact: a power of two, the result below 2^(M + 16)),
// truncated, plus r; n = 2^M is the smallest normal.  The sign of q stays, on a zero too.  The element conversions
// (Fp8Fmt::cvt4, fp4_code, fp6_code) are exact on the result.
template <int F>
__device__ __forceinline__ float mx_sr(float q, uint32_t r)
{
    constexpr int M = MxGrid<F>::M, B = MxGrid<F>::bias;
    constexpr int sh = 23 - M;
    constexpr uint32_t one = (uint32_t)(128 - B) << 23;                 // bits of 2^(1 - B), the smallest normal
    const uint32_t a = abs_bits(q);
    const uint32_t f16 = (a >> (sh - 16)) & 0xffffu;
    const uint32_t nrm = ((a >> sh) + ((f16 + r) >> 16)) << sh;
    const uint32_t u = (uint32_t)(__uint_as_float(a) * __uint_as_float((uint32_t)(127 + 16 + B + M - 1) << 23));
    const uint32_t n = (u + r) >> 16;
    const uint32_t sub = __float_as_uint((float)n * __uint_as_float((uint32_t)(127 + 1 - B - M) << 23));
    return __uint_as_float((a >= one ? nrm : sub) | (__float_as_uint(q) & 0x80000000u));
}

// mx_code4 with elem = RNE(SR(q, r)): r the 16-bit draws of the four elements
template <int F>
__device__ __forceinline__ uint32_t mx_code4_sr(const float *v, uint32_t sc, const uint32_t *r)
{
    if (sc == 0xffu) return (F == FP8Q_MX_E2M1 || kFp6<F>) ? 0u : 0x7f7f7f7fu;
    const float inv = scale_inv(sc);
    const float q0 = mx_sr<F>(mx_q<F>(v[0], inv), r[0]), q1 = mx_sr<F>(mx_q<F>(v[1], inv), r[1]);
    const float q2 = mx_sr<F>(mx_q<F>(v[2], inv), r[2]), q3 = mx_sr<F>(mx_q<F>(v[3], inv), r[3]);
    return mx_pack4<F>(q0, q1, q2, q3);
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
