// fp8q_intepilogue.hip -- the producer epilogue (eval-BN + residual + ReLU/ReLU6, fp8q_affine.h) fused with the per-tensor
// uniform INT activation quantizer (fp8q_intq.h): the INT twin of fp8q_epilogue.hip's quantizing kernels.
//   t = fma(x, alpha_c, beta'_c)       the folded [C, 2] vector of fp8q_bn_fold_f32 (optional)
//   t = t + residual                   (optional)
//   t = relu(t) / relu6(t)             (optional; NaN stays NaN)          -- bn_ab / res_act
//   y = scale * (clamp(rint(t / scale) + zp, int_min, int_max) - zp)      -- int_one
// bit for bit fp8q_int_quantize_f32 applied to the output of fp8q_affine_act_f32, in one pass: 8 B / element (12 with a
// residual) instead of 24 (28) for batch_norm, activation and quantizer as three launches.
// Two kernels, a staged one and a one-group-per-lane one, as for the FP8 quantizer: the plane walk, the staged kernels' plane
// constants and the choice between the kernels are fp8q_affine.h's, shared with fp8q_epilogue.hip (whose kernels carry the
// measurements behind that geometry).  The uniform quantizer has no {s, 1/s} table: its constants {scale, 1/scale, zp} are
// consts_of() of two uniform-address loads and one division per thread, so there is no LDS table, no table barrier and no
// prepared block.  RANGE: (delta, zero_float, sign) come from (x_min[0], x_max[0]) by range_of() in every block, and block
// (0, 0) of the first launch reports them -- set_quant_range and the quantizer in one launch.
#include "fp8q_common.h"
#include "fp8q_affine.h"
#include "fp8q_intq.h"

namespace {

struct IntEpiArgs {
    const float *a;          // delta [1] | RANGE: x_min [1]
    const float *b;          // zero_float [1] (asymmetric) | RANGE: x_max [1]
    unsigned char *sflag;    // symmetric: the sign (read | RANGE: written)
    float *delta_out;        // RANGE: delta written here ...
    float *zf_out;           // ... and zero_float (asymmetric)
    int report;              // RANGE: this launch's block (0, 0) writes them
    int symmetric;
    float eps;
    IntGrid grid;
};

// what a thread reads of the launch's quantizer: uniform-address loads without a branch around them (the host points an
// unused `b` / `sflag` at `a`).  a and b are scalar loads.  The sign byte is a vector load: waiting for it waits for every
// vector load requested before it, so nothing but the grid ends depends on it (epi_consts below) and the one-group-per-lane
// kernel requests it BEHIND its x / residual / BN loads.
struct EpiRaw {
    float a, b;
};

__device__ __forceinline__ EpiRaw epi_load(const IntEpiArgs &q)
{
    return EpiRaw{q.a[0], q.b[0]};
}

// the quantizer's sign: RANGE from x_min, otherwise the device byte `flag` = q.sflag[0] (sign_byte())
template <bool RANGE>
__device__ __forceinline__ bool epi_sign(const IntEpiArgs &q, const EpiRaw &raw, unsigned char flag)
{
    return q.symmetric && (RANGE ? raw.a < 0.0f : flag != 0);
}

// {scale, 1/scale, zp}: the part of the quantizer that does NOT depend on the sign byte -- a symmetric quantizer has zp = 0
// whatever its sign, an asymmetric one is unsigned -- so its division can run while the loads are in flight
template <bool RANGE>
__device__ __forceinline__ float4 epi_consts(const IntEpiArgs &q, const EpiRaw &raw)
{
    const float lo = q.grid.lo(false), hi = q.grid.hi(false);      // the clamp of zp: asymmetric only
    if (RANGE) {
        const bool sgn = q.symmetric && raw.a < 0.0f;     // a NaN minimum: unsigned (int_sign's per-tensor fold)
        const Range r = range_of(raw.a, raw.b, q.symmetric, q.grid.hi(sgn), q.eps);
        if (q.report && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
            q.delta_out[0] = r.delta;
            if (q.symmetric) q.sflag[0] = (unsigned char)sgn;
            else q.zf_out[0] = r.zf;
        }
        return consts_of(r.delta, r.zf, q.symmetric, lo, hi, q.eps);
    }
    return consts_of(raw.a, q.symmetric ? 0.0f : raw.b, q.symmetric, lo, hi, q.eps);
}

// k_affine_act's skeleton: blockIdx.y = image, blockIdx.x strides over the image in aligned pieces of U * 1024 elements;
// the {alpha, beta'} of the planes a piece overlaps in LDS, or in registers when it overlaps at most two.  x, residual and
// y are not __restrict__: y may be either of the other two (a lane reads an index before it writes it, and no other does).
template <bool RANGE, bool NT, int U>
__global__ void __launch_bounds__(kBlock)
k_int_affine_act(const float *x, const float *res, float *y, const float *__restrict__ ab, IntEpiArgs q, AffineArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *cst = reinterpret_cast<float2 *>(smem);   // [cpp] {alpha, beta'} (has_bn only)
    const int tid = threadIdx.x;
    const EpiRaw raw = epi_load(q);
    const float4 k = epi_consts<RANGE>(q, raw);
    const bool sgn = epi_sign<RANGE>(q, raw, RANGE ? (unsigned char)0 : q.sflag[0]);
    const float lo = q.grid.lo(sgn), hi = q.grid.hi(sgn);
    const int64_t base0 = (int64_t)blockIdx.y * a.image;
    const int nvec = (int)(a.image >> 2);
    const vf4 *xv = reinterpret_cast<const vf4 *>(x + base0);
    const vf4 *rv = reinterpret_cast<const vf4 *>(res + (a.has_res ? base0 : 0));
    vf4 *yv = reinterpret_cast<vf4 *>(y + base0);
    const uint32_t HW = (uint32_t)a.HW;
    const bool direct = affine_direct(a);
    for (int base = blockIdx.x * (kBlock * U); base < nvec; base += gridDim.x * (kBlock * U)) {
        float2 p0, p1;
        const uint32_t phase = affine_step_planes(base, direct, a, p0, p1, cst, [&](uint32_t ch) {
            return bn_ab(ab, nullptr, nullptr, nullptr, ch, 2);
        });
        // the epilogue and the quantizer of one 16-byte group; g: piece-local group index
        auto finish = [&](int g, const vf4 &v, const vf4 &r) -> vf4 {
            float e[4] = {v.x, v.y, v.z, v.w};
            const float rr[4] = {r.x, r.y, r.z, r.w};
            if (direct) {
                const uint32_t o = phase + 4u * (uint32_t)g;
                const bool up = o >= HW;                    // second plane of the piece
                affine_walk(e, rr, up ? o - HW : o, HW, up ? p1 : p0, a, [&] { return p1; });
            } else if (a.has_bn) {
                const uint32_t o = phase + 4u * (uint32_t)g;
                uint32_t lch = affine_local_plane(o, a);
                affine_walk(e, rr, o - lch * HW, HW, cst[lch], a, [&] { return cst[++lch]; });
            } else {
                affine_plain(e, rr, a);
            }
            return vf4{int_one(e[0], k, lo, hi), int_one(e[1], k, lo, hi), int_one(e[2], k, lo, hi), int_one(e[3], k, lo, hi)};
        };
        const vf4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        if (base + kBlock * U <= nvec) {   // whole piece: unpredicated loads, all of them in flight
            vf4 vx[U], vr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) vx[u] = ld16<NT>(xv + base + u * kBlock + tid);
#pragma unroll
            for (int u = 0; u < U; ++u) vr[u] = a.has_res ? ld16<NT>(rv + base + u * kBlock + tid) : zero;
            vf4 out[U];
#pragma unroll
            for (int u = 0; u < U; ++u) out[u] = finish(u * kBlock + tid, vx[u], vr[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) st16<NT>(yv + base + u * kBlock + tid, out[u]);
        } else {
            for (int u = 0; u < U; ++u) {
                const int j = base + u * kBlock + tid;
                if (j >= nvec) break;
                const vf4 v = ld16<NT>(xv + j);
                const vf4 r = a.has_res ? ld16<NT>(rv + j) : zero;
                st16<NT>(yv + j, finish(u * kBlock + tid, v, r));
            }
        }
    }
}

// k_affine_act_small's skeleton for cache-sized tensors (latency-bound: what counts is the dependent chain from block start
// to the first store): one 16-byte group per lane and step, the {alpha, beta'} of the group's plane and of the next one
// straight from global memory (HW >= 4: a group spans at most two planes).  x, residual and the BN constants of the first
// group are requested BEFORE the quantizer's constants are formed, so that the range arithmetic and the division of
// consts_of() run while those loads are in flight; the next group is requested behind the store of the current one.
template <bool RANGE>
__global__ void __launch_bounds__(kBlock)
k_int_affine_act_small(const float *x, const float *res, float *y, const float *__restrict__ ab, IntEpiArgs q, AffineArgs a)
{
    const int tid = threadIdx.x;
    const int64_t base0 = (int64_t)blockIdx.y * a.image;
    const int nvec = (int)(a.image >> 2);
    const vf4 *xv = reinterpret_cast<const vf4 *>(x + base0);
    const vf4 *rv = reinterpret_cast<const vf4 *>(res + (a.has_res ? base0 : 0));
    vf4 *yv = reinterpret_cast<vf4 *>(y + base0);
    const int step = gridDim.x * kBlock;
    int j = blockIdx.x * kBlock + tid;
    const EpiRaw raw = epi_load(q);
    AffineGrp g;
    if (j < nvec) affine_fetch(g, xv, rv, j, ab, nullptr, nullptr, nullptr, 2, a);
    const unsigned char flag = RANGE ? (unsigned char)0 : q.sflag[0];     // requested last: waiting for it waits for all
    const float4 k = epi_consts<RANGE>(q, raw);       // (used in the loop only, defined in front of it: stays in front of the wait)
    while (j < nvec) {
        float e[4];
        affine_apply(g, e, a);
        const bool sgn = epi_sign<RANGE>(q, raw, flag);
        const float lo = q.grid.lo(sgn), hi = q.grid.hi(sgn);
        yv[j] = vf4{int_one(e[0], k, lo, hi), int_one(e[1], k, lo, hi), int_one(e[2], k, lo, hi), int_one(e[3], k, lo, hi)};
        j += step;
        if (j < nvec) affine_fetch(g, xv, rv, j, ab, nullptr, nullptr, nullptr, 2, a);
    }
}

// argument checks (affine_args, make_int_grid), then affine_dispatch's kernel; the first launch reports a RANGE
template <bool RANGE>
int int_affine_launch(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW, const float *alpha_beta,
                      int act, IntEpiArgs q, int n_bits, hipStream_t st)
{
    AffineArgs a;
    if (int rc = affine_args(N, C, HW, act, alpha_beta ? 2 : 0, residual != nullptr, &a)) return rc;
    if (int rc = make_int_grid(n_bits, q.grid)) return rc;
    if (N == 0) return FP8Q_OK;
    if (!x || !y || !q.a || (q.symmetric ? !q.sflag : !q.b)) return FP8Q_EINVAL;
    if (RANGE && (!q.b || !q.delta_out || (!q.symmetric && !q.zf_out))) return FP8Q_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)residual) & 15) || ((uintptr_t)alpha_beta & 7) ||
        (((uintptr_t)q.a | (uintptr_t)q.b | (uintptr_t)q.delta_out | (uintptr_t)q.zf_out) & 3))
        return FP8Q_EINVAL;
    if (!q.b) q.b = q.a;                                             // never used: read, so that no load sits behind a branch
    if (!q.sflag) q.sflag = reinterpret_cast<unsigned char *>(const_cast<float *>(q.a));
    affine_dispatch(N, a, false, [&](AffineKernel kind, dim3 g, size_t shm, int64_t n0) {
        const float *xp = x + n0 * a.image, *rp = residual ? residual + n0 * a.image : nullptr;
        float *yp = y + n0 * a.image;
        q.report = n0 == 0;
        hipLaunchKernelGGL((kind == AffineKernel::StagedNt  ? k_int_affine_act<RANGE, true, 4>
                            : kind == AffineKernel::Small   ? k_int_affine_act_small<RANGE>
                            : kind == AffineKernel::Staged1 ? k_int_affine_act<RANGE, false, 1> : k_int_affine_act<RANGE, false, 4>),
                           g, dim3(kBlock), shm, st, xp, rp, yp, alpha_beta, q, a);
    });
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_int_affine_act_quantize_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW,
                                     const float *alpha_beta, int act, const float *delta, const float *zero_float,
                                     const unsigned char *signed_flag, int n_bits, int symmetric, float eps,
                                     fp8q_stream_t stream)
{
    IntEpiArgs q = {};
    q.a = delta;
    q.b = zero_float;
    q.sflag = const_cast<unsigned char *>(signed_flag);   // read only (RANGE == false)
    q.symmetric = symmetric != 0;
    q.eps = eps;
    return int_affine_launch<false>(x, residual, y, N, C, HW, alpha_beta, act, q, n_bits, (hipStream_t)stream);
}

int fp8q_int_affine_act_range_quantize_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW,
                                           const float *alpha_beta, int act, const float *x_min, const float *x_max,
                                           float *delta_out, float *zero_float_out, unsigned char *signed_flag_out, int n_bits,
                                           int symmetric, float eps, fp8q_stream_t stream)
{
    IntEpiArgs q = {};
    q.a = x_min;
    q.b = x_max;
    q.sflag = signed_flag_out;
    q.delta_out = delta_out;
    q.zf_out = zero_float_out;
    q.symmetric = symmetric != 0;
    q.eps = eps;
    return int_affine_launch<true>(x, residual, y, N, C, HW, alpha_beta, act, q, n_bits, (hipStream_t)stream);
}

}  // extern "C"
