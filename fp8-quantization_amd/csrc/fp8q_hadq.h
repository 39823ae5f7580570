// fp8q_hadq.h -- the device arithmetic of the block Hadamard rotation (gfx950 only), shared by fp8q_mx_had.hip (blocks along the
// last dimension) and fp8q_mx_had_t.hip (blocks along dim 0).  The contract is stated once, in include/fp8q.h:
//   signs        v[i] ^= bit i of sign_mask << 31, an exact flip (zeros, infinities and NaNs too)
//   butterflies  stages s = 0 .. 4; for i with bit s clear, j = i | 1 << s: (v[i], v[j]) <- (fl32(v[i] + v[j]), fl32(v[i] - v[j]))
//   norm         one fp32 multiplication by kHadNorm = 0x3E3504F3, the float32 nearest to 2^-2.5
// and the inverse runs butterflies, norm, signs.  No fused multiply-add: nothing here is of the form a * b + c (and the library
// is compiled with -ffp-contract=off).
// Why butterflies and not the matrix cores: (1) the accumulation order of a v_mfma_* instruction is not specified, so no
// byte-exact contract could be stated, and this project states one for every lane; (2) 160 additions per block against 1024
// multiply-adds -- even at the float32 matrix rate the kernels would be bound by arithmetic rather than by HBM.
// A block lies across lanes the way the MX kernels hold it, so some stages are in registers (had_regs) and the others one
// exchange with the lane STEP away by xor (had_cross): DPP moves for 1, 2 and 4 as umax_xor makes them, ds_bpermute for 16 and
// 32 as k_mxt's column maxima do.  The upper lane of a pair needs theirs - mine: its own value goes in with the sign flipped
// and the one addition is theirs + (-mine), which IS that subtraction in IEEE arithmetic, the sign of a zero result included.
// Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"
#include "fp8q_mxq.h"

namespace {

constexpr uint32_t kHadNormBits = 0x3E3504F3u;

// the signs of N consecutive elements of a block: bit j of `bits` flips v[j * ST] (higher bits of `bits` are ignored)
template <int N, int ST = 1>
__device__ __forceinline__ void had_signs(float *v, uint32_t bits)
{
#pragma unroll
    for (int j = 0; j < N; ++j) v[j * ST] = __uint_as_float(__float_as_uint(v[j * ST]) ^ ((bits >> j) << 31));
}

// the log2(N) stages whose pairs lie in the lane's N registers (ST apart), lowest stride first
template <int N, int ST = 1>
__device__ __forceinline__ void had_regs(float *v)
{
#pragma unroll
    for (int s = 1; s < N; s <<= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i & s) continue;
            const float lo = v[i * ST], hi = v[(i | s) * ST];
            v[i * ST] = lo + hi;
            v[(i | s) * ST] = lo - hi;
        }
    }
}

template <int CTRL>
__device__ __forceinline__ float had_dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// the value of the lane STEP away by xor (every lane of the wave is live where this runs).  4: row_half_mirror (lane i <->
// i ^ 7 of its 8), then the quad reversed (i ^ 3)
template <int STEP>
__device__ __forceinline__ float had_partner(float v)
{
    if constexpr (STEP == 1) return had_dpp<0xB1>(v);
    else if constexpr (STEP == 2) return had_dpp<0x4E>(v);
    else if constexpr (STEP == 4) return had_dpp<0x1B>(had_dpp<0x141>(v));
    else return __shfl_xor(v, STEP);
}

// one stage across lanes for N registers; neg: 0x80000000 in the lane that holds the upper elements of its pairs, else 0
template <int STEP, int N>
__device__ __forceinline__ void had_cross(float *v, uint32_t neg)
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float o = had_partner<STEP>(v[j]);
        v[j] = o + __uint_as_float(__float_as_uint(v[j]) ^ neg);
    }
}

template <int N>
__device__ __forceinline__ void had_norm(float *v)
{
    const float c = __uint_as_float(kHadNormBits);
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] *= c;
}

// a whole block in one lane (the general routes): signs `pre` before, signs `post` after -- (mask, 0) is the rotation,
// (0, mask) its inverse
__device__ __forceinline__ void had_block32(float *v, uint32_t pre, uint32_t post)
{
    had_signs<32>(v, pre);
    had_regs<32>(v);
    had_norm<32>(v);
    had_signs<32>(v, post);
}

// host side: the `sr, seed, offset` of an fp8q_mxh_* entry.  sr_on is 0 (round to nearest even: *use is null and the seed and
// offset are not read) or 1
inline int had_sr_args(int sr_on, uint64_t seed, uint64_t offset, MxSr *sr, const MxSr **use)
{
    if (sr_on != 0 && sr_on != 1) return FP8Q_EINVAL;
    *sr = mx_sr_args(seed, offset);
    *use = sr_on ? sr : nullptr;
    return FP8Q_OK;
}

}  // namespace
