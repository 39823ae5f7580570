// fp8q_affine.h -- what the producer epilogues share (fp8q_epilogue.hip: BN + residual + activation in front of the FP8
// quantizer, its quantizer-less form and its calibration twin; fp8q_intepilogue.hip: the same epilogue in front of the
// uniform INT quantizers): the geometry block of an [N, C, HW] tensor, the folded batch-norm constants of a channel, the
// residual + activation step, the argument checks, the launch grid and the small-tensor threshold.  Internal linkage, as
// fp8q_common.h.
#pragma once
#include "fp8q_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// N2: producer epilogue fused with the activation quantizer:
//   t = fma(x, alpha_c, fma(-mean_c, alpha_c, beta_c)), alpha_c = invstd_c * gamma_c   (eval-mode BN, NCHW)
//   t = t + residual                                          (optional)
//   t = relu(t) / relu6(t)                                    (optional)
//   QUANT:  y = quantize_to_fp8(t; per-tensor maxval)        MINMAX: min/max of t -> partials
// i.e. quantized_folded_bn.py:39-55 and models/resnet_quantized.py:43-46 in one pass (8 B/element
// instead of three 8 B passes).  Flat over N*C*HW; channel of a 16-byte group by two magic
// divisions, per element only when a group crosses a plane boundary (HW % 4 != 0).
// ---------------------------------------------------------------------------------------------
struct AffineArgs {
    int64_t image;      // C * HW elements per image (multiple of 4, < 2^31)
    int C, HW;
    int act;            // 0 none, 1 relu, 2 relu6
    int has_bn, has_res;
    int cpp;            // most channels one 4096-element piece can overlap (size of the LDS constants)
    uint32_t magic;     // o / HW for o < 4096 + HW (magic_of); unused when HW > kAffineMagicMaxHW
    uint64_t magic48;   // floor(2^48 / HW) + 1:  n / HW == (n * magic48) >> 48  for n * HW < 2^48 (calibration twin)
    int passthrough;    // y = t itself, no quantizer (fp8q_affine_act_f32: what an MSE estimator searches on; maxval unused)
};
constexpr int kAffinePiece = kBlock * 4 * 4;   // elements per block and step (16 KiB)
constexpr int kAffineMagicMaxHW = kMagicMaxDivisor;   // above: a piece spans <= 2 planes (compare instead of divide)

// {alpha, beta'} of one channel: alpha = invstd * gamma, beta' = fma(-mean, alpha, beta) (ATen's eval-mode batch norm) --
// or, with has_bn == 2, read from the folded [C, 2] vector that fp8q_bn_fold_f32 wrote (`mean` then points to it): one
// 8-byte load instead of four 4-byte ones per plane, the same two numbers.
__device__ __forceinline__ float2 bn_ab(const float *__restrict__ mean, const float *__restrict__ invstd,
                                        const float *__restrict__ gamma, const float *__restrict__ beta, uint32_t ch, int has_bn)
{
    if (has_bn == 2) return reinterpret_cast<const float2 *>(mean)[ch];
    const float alpha = invstd[ch] * gamma[ch];
    return make_float2(alpha, fmaf(-mean[ch], alpha, beta[ch]));
}

// act(t + r) -- the non-affine part of the epilogue
__device__ __forceinline__ float res_act(float t, float r, const AffineArgs &a)
{
    if (a.has_res) t = t + r;
    if (a.act >= 1) t = t < 0.0f ? 0.0f : t;         // NaN stays NaN (torch.relu)
    if (a.act == 2) t = t > 6.0f ? 6.0f : t;
    return t;
}

// ---- host side ----
inline int affine_args(int64_t N, int64_t C, int64_t HW, int act, int has_bn, bool has_res, AffineArgs *a)
{
    if (N < 0 || C <= 0 || HW <= 0 || act < 0 || act > 2) return FP8Q_EINVAL;
    // 16-byte groups must not straddle images; 32-bit element indices within an image; the 48-bit magic
    // division of the calibration twin needs C*HW*HW < 2^48
    if (((C * HW) & 3) != 0 || C * HW >= (1ll << 31) || HW >= (1 << 24) ||
        (double)C * (double)HW * (double)HW >= 281474976710656.0)
        return FP8Q_EUNSUPPORTED;
    a->image = C * HW;
    a->C = (int)C;
    a->HW = (int)HW;
    a->act = act;
    a->has_bn = has_bn;
    a->has_res = has_res;
    const int64_t cpp = (HW + kAffinePiece - 2) / HW + 1;   // planes a 4096-element window can overlap
    a->cpp = (int)(cpp < C ? cpp : C);
    a->magic = HW <= kAffineMagicMaxHW ? magic_of((int)HW) : 0u;
    a->magic48 = (1ull << 48) / (uint64_t)HW + 1ull;
    a->passthrough = 0;
    return FP8Q_OK;
}

inline void affine_grid(int64_t N, const AffineArgs &a, bool quant, int64_t *bx, int64_t *by, int U = 4)
{
    const int64_t ymax = quant ? 65535 : 65534;   // the calibration twin adds one block row for its reducer
    *by = N < ymax ? N : ymax;
    const int64_t nvec = a.image >> 2;
    if (quant) {
        // one 16 KiB piece per block while the grid stays below 64 K blocks; a partial last piece of the
        // image gets no block of its own
        const int64_t pieces = nvec / (kBlock * U) > 0 ? nvec / (kBlock * U) : 1;
        static const int64_t cap_env = [] {   // FP8Q_EPI_GRID: total block cap of the quantizing epilogue kernel (experiments)
            const char *e = getenv("FP8Q_EPI_GRID");
            const long v = e ? atol(e) : 0;
            return (int64_t)(v > 0 ? v : 0);
        }();
        // tensors beyond the caches: one piece per block; cache-sized ones (< 64 MiB): a resident grid of 2048 blocks with
        // the same number of pieces each -- one piece per block is then a handful of ROUNDS of the resident blocks, and a
        // fractional last round is lost time ([64,144,28,28] 20.2 -> 17.0 us, [64,24,56,56] 15.8 -> 13.8, [64,64,56,56]
        // 25.2 -> 23.7, [64,128,28,28] 18.5 -> 16.9 by rocprofv3)
        const bool cache_sized = N * a.image * 4 < kNtBytes;
        const int64_t total = cap_env ? cap_env : ((cache_sized || pieces * *by <= 4096) ? kTargetBlocks : 65536);
        *bx = balanced_blocks(pieces, total / *by > 0 ? total / *by : 1);   // K1's grid rule
    } else {
        // read-only twin: a persistent grid of <= 2048 blocks with 4 KiB steps measured best (36 us against
        // 43-55 us for 16 KiB steps or one piece per block at [64,64,112,112])
        int64_t b = cdiv(nvec, kBlock * 4);
        const int64_t cap = kTargetBlocks / *by > 0 ? kTargetBlocks / *by : 1;
        *bx = b > cap ? cap : (b < 1 ? 1 : b);
    }
}

// FP8Q_EPI_SMALL_M: tensors below this many M elements run 4 KiB pieces per block (cache-sized tensors are
// latency-bound: four times as many blocks with a quarter of the piece each)
inline int64_t affine_small_elems()
{
    static const int64_t v = [] {
        const char *e = getenv("FP8Q_EPI_SMALL_M");
        const long m = e ? atol(e) : -1;
        return (int64_t)(m >= 0 ? m : 16) << 20;
    }();
    return v;
}

}  // namespace
