// fp8q_affine.h -- what the producer epilogues share (fp8q_epilogue.hip: BN + residual + activation in front of the FP8
// quantizer, its quantizer-less form and its calibration twin; fp8q_intepilogue.hip: the same epilogue in front of the
// uniform INT quantizers): the geometry block of an [N, C, HW] tensor, the folded batch-norm constants of a channel, the
// residual + activation step, the walk of a 16-byte group across a plane border (affine_walk: constants reloaded at the
// border; AffineGrp / affine_fetch / affine_apply: both planes' constants fetched with the group, picked branch-free), the
// per-step plane constants of the staged kernels (affine_step_planes, affine_local_plane), the argument checks, the launch
// grid, the small-tensor threshold and the choice of kernel (affine_dispatch).  Internal linkage, as fp8q_common.h.
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

// The staged kernels behind a batch norm keep the constants of a piece's planes in registers when there are at most two
// (`direct`: uniform addresses, scalar loads) and stage them in LDS otherwise.  One rule for the FP8 and the INT kernel and
// for fp8q_affine_act_route, which reports it.
__host__ __device__ __forceinline__ bool affine_direct(const AffineArgs &a)
{
    return a.has_bn && a.cpp <= 2;
}

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

// The four elements of one 16-byte group whose first element sits at offset `off` of a plane with constants p = {alpha,
// beta'}: e = act(fma(e, alpha, beta') + rr), rr the group's residuals.  HW % 4 != 0: the group may cross into the next plane (and, HW < 4, into
// further ones), whose constants next() yields -- still inside the image, since groups never straddle images, so there IS
// a next plane whenever next() is called.
template <class Next>
__device__ __forceinline__ void affine_walk(float (&e)[4], const float (&rr)[4], uint32_t off, uint32_t HW, float2 p,
                                            const AffineArgs &a, Next next)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        e[k] = res_act(fmaf(e[k], p.x, p.y), rr[k], a);
        if (++off == HW && k < 3) {
            off = 0;
            p = next();
        }
    }
}

// ... and without a batch norm
__device__ __forceinline__ void affine_plain(float (&e)[4], const float (&rr)[4], const AffineArgs &a)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = res_act(e[k], rr[k], a);
}

// One 16-byte group of the one-group-per-lane kernels with everything its epilogue reads, requested together
struct AffineGrp {
    vf4 v, r;
    float2 q0, q1;    // {alpha, beta'} of the group's plane and of the next one (HW >= 4: a group spans <= 2)
    uint32_t off;     // offset of the group's first element inside its plane
};

// group jj of an image; bn: the has_bn of bn_ab (the vectors are read only with a.has_bn)
__device__ __forceinline__ void affine_fetch(AffineGrp &g, const vf4 *xv, const vf4 *rv, int jj, const float *mean,
                                             const float *invstd, const float *gamma, const float *beta, int bn,
                                             const AffineArgs &a)
{
    g.v = xv[jj];
    g.r = a.has_res ? rv[jj] : vf4{0.0f, 0.0f, 0.0f, 0.0f};
    g.off = 0;
    g.q0 = g.q1 = make_float2(1.0f, 0.0f);
    if (a.has_bn) {
        const uint32_t i0 = (uint32_t)jj * 4u;
        const uint32_t ch = (uint32_t)(((uint64_t)i0 * a.magic48) >> 48);      // plane == channel
        g.off = i0 - ch * (uint32_t)a.HW;
        g.q0 = bn_ab(mean, invstd, gamma, beta, ch, bn);
        g.q1 = bn_ab(mean, invstd, gamma, beta, ch + 1u < (uint32_t)a.C ? ch + 1u : ch, bn);
    }
}

// e = the epilogue of the group's four elements
__device__ __forceinline__ void affine_apply(const AffineGrp &g, float (&e)[4], const AffineArgs &a)
{
    e[0] = g.v.x, e[1] = g.v.y, e[2] = g.v.z, e[3] = g.v.w;
    const float rr[4] = {g.r.x, g.r.y, g.r.z, g.r.w};
    if (a.has_bn) {
        // elements at group-local index >= cross belong to the next plane (HW >= 4: at most one crossing)
        const uint32_t cross = (uint32_t)a.HW - g.off;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool nxt = (uint32_t)k >= cross;
            e[k] = res_act(fmaf(e[k], nxt ? g.q1.x : g.q0.x, nxt ? g.q1.y : g.q0.y), rr[k], a);
        }
    } else {
        affine_plain(e, rr, a);
    }
}

// The staged kernels' step over the piece that starts at group `base` of the image: returns the offset of the piece's
// first element inside its plane and leaves the constants of the planes the piece overlaps -- `direct` (at most two
// planes): in p0 / p1, uniform addresses, i.e. scalar loads; otherwise in cst[0 .. cpp), between two barriers (the first:
// the previous step's constants are no longer read).  plane(ch): the constants of channel ch.  (Two separate branches, each
// with its own division, and in the callers the group's offset formed inside each branch: with this shape the compiler gives
// k_affine_act the instruction stream it had when the code was local; one nested branch and one hoisted offset grew the
// U = 4 kernels by 3 % in instructions and measured 1 % slower at [64,64,112,112].)
template <class Plane>
__device__ __forceinline__ uint32_t affine_step_planes(int base, bool direct, const AffineArgs &a, float2 &p0, float2 &p1,
                                                       float2 *cst, Plane plane)
{
    const uint32_t HW = (uint32_t)a.HW;
    uint32_t phase = 0;
    p0 = make_float2(1.0f, 0.0f), p1 = p0;
    if (direct) {
        const uint32_t e0 = (uint32_t)base * 4u;
        const uint32_t ch_lo = e0 / HW;
        phase = e0 - ch_lo * HW;
        const uint32_t ch_hi = ch_lo + 1u < (uint32_t)a.C ? ch_lo + 1u : ch_lo;
        p0 = plane(ch_lo);
        p1 = plane(ch_hi);
    }
    if (a.has_bn && !direct) {
        __syncthreads();
        const uint32_t e0 = (uint32_t)base * 4u;
        const uint32_t ch_lo = e0 / HW;
        phase = e0 - ch_lo * HW;
        for (int k = threadIdx.x; k < a.cpp; k += kBlock) {
            const uint32_t ch = ch_lo + (uint32_t)k;
            if (ch < (uint32_t)a.C) cst[k] = plane(ch);
        }
        __syncthreads();
    }
    return phase;
}

// index into cst of the plane that holds piece-local offset o (o counted from the first staged plane's start).  A plane
// beyond the magic division's range is longer than a piece, so the piece overlaps two planes and a compare does it
// (such a piece has cpp <= 2 and is `direct` in both staged kernels today: the compare guards div_small's range)
__device__ __forceinline__ uint32_t affine_local_plane(uint32_t o, const AffineArgs &a)
{
    return (uint32_t)a.HW > (uint32_t)kAffineMagicMaxHW ? (o >= (uint32_t)a.HW ? 1u : 0u) : (uint32_t)div_small(o, a.magic);
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

// Which quantizing kernel serves a tensor, and its launches.  From 64 MiB (kNtBytes): the staged kernel, nontemporal, 16 KiB
// pieces.  Below the small-tensor threshold: the one-group-per-lane kernel -- or, HW < 4 behind a batch norm (a group can
// span more than two planes), the staged kernel with a group per lane.  In between (reached only with FP8Q_EPI_SMALL_M
// below FP8Q_NT_MB's 16 Mi elements): the staged kernel, 16 KiB pieces.  More than 65535 images: one launch per 65535.
// launch(kind, grid, dynamic LDS bytes, n0) starts the caller's kernel of that kind on the images from n0 on.
// small_grid_nt: a tensor that is nontemporal AND small (only with the two knobs set against each other) gets its grid
// sized for one group per lane although the nontemporal kernel strides by four -- the FP8 lane's behaviour; the INT lane
// sizes it for four.
enum class AffineKernel { StagedNt, Small, Staged1, Staged4 };

template <class Launch>
inline void affine_dispatch(int64_t N, const AffineArgs &a, bool small_grid_nt, Launch launch)
{
    const bool small = N * a.image < affine_small_elems();
    const bool nt = N * a.image * 4 >= kNtBytes;
    const AffineKernel kind = nt ? AffineKernel::StagedNt
                              : small && (a.HW >= 4 || !a.has_bn) ? AffineKernel::Small
                              : small ? AffineKernel::Staged1 : AffineKernel::Staged4;
    const size_t shm = a.has_bn && kind != AffineKernel::Small ? (size_t)a.cpp * sizeof(float2) : 0;
    for (int64_t n0 = 0; n0 < N; n0 += 65535) {
        int64_t bx, by;
        affine_grid(N - n0, a, true, &bx, &by, small && (small_grid_nt || !nt) ? 1 : 4);
        launch(kind, dim3((unsigned)bx, (unsigned)by), shm, n0);
    }
}

}  // namespace
