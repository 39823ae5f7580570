// fp8q_intgrad.hip -- backward of the uniform (INT) fake-quantizers (uniform_quantizers.py:108-164, linear scale domain,
// round_ste) in one streaming pass: d/dx, d/ddelta and d/dzero_float from x and the upstream gradient g
// (include/fp8q.h: fp8q_int_quantize_bwd_f32).
//
// Per element, in fp32, with the forward's own values (fp8q_int.hip: scale = max(delta, eps), zp, [lo, hi]):
//     t = x / scale  (the IEEE quotient, so rint(t) is the forward's rounding bit for bit: its reciprocal shortcut
//                     redoes exactly the lanes on which the two could differ)
//     u = rint(t) + zp,   m = [lo <= u <= hi]  (0 for a NaN u),   v = clamp(u, lo, hi)
//     gx = g * m
//     gdelta[row]      = [delta >= eps] sum g * w,   w = (v - zp) - m * t      (m * t: 0 * inf = NaN for x = +-inf, as
//                                                                               the autograd chain's 0 * ((x/scale)/scale))
//     gzero_float[row] = -[lo <= rint(zero_float) <= hi] sum (1 - m) * (g * scale)
// The products are fp32, the sums fp64.  LSQ's gradient scaling multiplies the two finished fp32 sums by
// gs = 1 / sqrt(hi * grad_scale_elems): both candidates (hi of the unsigned and of the signed grid) come from the host,
// the kernel picks by the device-resident sign.
//
// Geometry, reductions and the workspace rule are those of fp8q_grad.hip (fp8q_bwd.h): deterministic, no floating-point
// atomics, the finishing launch zeroes every word it has read.
//   k_igrad_rows    per tensor, and per-channel rows longer than kShortMaxInner: a block = (row, split); split s streams
//                   the 16 KiB pieces s, s + nsplit, ... of its row.
//   k_igrad_short   per-channel rows up to kShortMaxInner elements: G lanes own a row; both sums are finished in the wave.
//   k_igrad_final   block r: the split partials of row r in index order, then the masks and gs.
// All accesses are 16 bytes per lane at 4-byte alignment; the <= 3 elements behind a row's last group go one by one.
#include "fp8q_common.h"
#include "fp8q_bwd.h"
#include "fp8q_intq.h"

namespace {

struct IGradArgs {
    const float *delta;            // [n_delta]
    const float *zf;               // [n_delta], asymmetric
    const unsigned char *sflag;    // symmetric: the quantizer's sign
    int symmetric;
    int scaled;                    // grad_scale_elems > 0
    float eps;
    IntGrid grid;
    float gs_u, gs_s;              // gs for hi = n_hi_u / n_hi_s
};

// the integer grid and its gs
struct IGrid {
    float lo, hi, gs;
};

__device__ __forceinline__ IGrid igrad_grid(const IGradArgs &a)
{
    const bool sgn = sign_byte(a.symmetric, a.sflag);
    return IGrid{a.grid.lo(sgn), a.grid.hi(sgn), sgn ? a.gs_s : a.gs_u};
}

// one element: returns gx, adds its terms to the two sums; k = consts_of: {scale, -, zp, -}
template <bool SUMS>
__device__ __forceinline__ float igrad_elem(float x, float g, const float4 k, float lo, float hi, double &sa, double &sb)
{
    const float t = x / k.x;
    const float u = rintf(t) + k.z;
    const float m = ((u >= lo) & (u <= hi)) ? 1.0f : 0.0f;
    if (SUMS) {
        const float v = t_clamp(u, lo, hi);
        const float w = (v - k.z) - m * t;
        sa += (double)(g * w);
        sb += (double)((1.0f - m) * (g * k.x));
    }
    return g * m;
}

// a row's finished sums -> its two gradients
__device__ __forceinline__ void igrad_store(double sa, double sb, int64_t row, const IGradArgs &a, const IGrid &q,
                                            float *gdelta, float *gzero)
{
    if (gdelta) {
        float r = a.delta[row] >= a.eps ? (float)sa : 0.0f;      // clamp(delta, min = eps) passes the gradient from eps up
        if (a.scaled) r = r * q.gs;
        gdelta[row] = r;
    }
    if (gzero) {
        const float rz = rintf(a.zf[row]);                       // round_ste passes it, the clamp cuts it off outside
        float r = ((rz >= q.lo) & (rz <= q.hi)) ? -(float)sb : 0.0f;
        if (a.scaled) r = r * q.gs;
        gzero[row] = r;
    }
}

// ---------------------------------------------------------------------------------------------
// long rows: block = (row, split)
// ---------------------------------------------------------------------------------------------
template <bool NT, int U, bool SUMS>
__global__ void __launch_bounds__(kBlock)
k_igrad_rows(const float *__restrict__ x, const float *__restrict__ g, float *__restrict__ gx, int64_t inner, int nsplit,
             IGradArgs a, float *gdelta, float *gzero, double *part_a, double *part_b)
{
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x / (unsigned)nsplit;
    const int split = (int)(blockIdx.x - row * nsplit);
    const IGrid q = igrad_grid(a);
    const float4 k = consts_of(a.delta[row], a.symmetric ? 0.0f : a.zf[row], a.symmetric != 0, q.lo, q.hi, a.eps);
    const float *xr = x + row * inner;
    const float *gr = g + row * inner;
    float *or_ = gx ? gx + row * inner : nullptr;
    double sa = 0.0, sb = 0.0;

    const int64_t nvec = inner >> 2;
    const int64_t step = (int64_t)nsplit * (kBlock * U);
    for (int64_t base = (int64_t)split * (kBlock * U); base < nvec; base += step) {
        if (base + kBlock * U <= nvec) {
            vf4 xv[U], gv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                xv[u] = ld16u<NT>(xr + 4 * (base + u * kBlock + tid));
                gv[u] = ld16u<NT>(gr + 4 * (base + u * kBlock + tid));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                vf4 o;
                o.x = igrad_elem<SUMS>(xv[u].x, gv[u].x, k, q.lo, q.hi, sa, sb);
                o.y = igrad_elem<SUMS>(xv[u].y, gv[u].y, k, q.lo, q.hi, sa, sb);
                o.z = igrad_elem<SUMS>(xv[u].z, gv[u].z, k, q.lo, q.hi, sa, sb);
                o.w = igrad_elem<SUMS>(xv[u].w, gv[u].w, k, q.lo, q.hi, sa, sb);
                if (or_) st16u<NT>(or_ + 4 * (base + u * kBlock + tid), o);
            }
        } else {
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + u * kBlock + tid;
                if (i < nvec) {
                    const vf4 xv = ld16u<NT>(xr + 4 * i), gv = ld16u<NT>(gr + 4 * i);
                    vf4 o;
                    o.x = igrad_elem<SUMS>(xv.x, gv.x, k, q.lo, q.hi, sa, sb);
                    o.y = igrad_elem<SUMS>(xv.y, gv.y, k, q.lo, q.hi, sa, sb);
                    o.z = igrad_elem<SUMS>(xv.z, gv.z, k, q.lo, q.hi, sa, sb);
                    o.w = igrad_elem<SUMS>(xv.w, gv.w, k, q.lo, q.hi, sa, sb);
                    if (or_) st16u<NT>(or_ + 4 * i, o);
                }
            }
        }
    }
    if (split == 0) {                         // the <= 3 elements behind the last 16-byte group of the row
        const int64_t t = (nvec << 2) + tid;
        if (t < inner) {
            const float o = igrad_elem<SUMS>(xr[t], gr[t], k, q.lo, q.hi, sa, sb);
            if (or_) or_[t] = o;
        }
    }
    if (SUMS) {
        block_sum2(sa, sb);
        if (tid == 0) {
            if (nsplit == 1) {
                igrad_store(sa, sb, row, a, q, gdelta, gzero);
            } else {
                if (part_a) part_a[blockIdx.x] = sa;
                if (part_b) part_b[blockIdx.x] = sb;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// short rows: G lanes own a row
// ---------------------------------------------------------------------------------------------
template <bool NT, bool SUMS>
__global__ void __launch_bounds__(kBlock)
k_igrad_short(const float *__restrict__ x, const float *__restrict__ g, float *__restrict__ gx, int64_t C, int inner, int G,
              IGradArgs a, float *gdelta, float *gzero)
{
    const int tid = threadIdx.x;
    const int sub = tid & (G - 1), slot = tid / G, rpp = kBlock / G;
    const IGrid q = igrad_grid(a);
    const int nvec = inner >> 2;
    const int64_t npass = (C + rpp - 1) / rpp;
    for (int64_t p = blockIdx.x; p < npass; p += gridDim.x) {
        const int64_t row = p * rpp + slot;
        const bool live = row < C;
        double sa = 0.0, sb = 0.0;
        if (live) {
            const float4 k = consts_of(a.delta[row], a.symmetric ? 0.0f : a.zf[row], a.symmetric != 0, q.lo, q.hi, a.eps);
            const float *xr = x + row * inner;
            const float *gr = g + row * inner;
            float *or_ = gx ? gx + row * inner : nullptr;
            constexpr int U = 4;
            for (int v0 = sub; v0 < nvec; v0 += U * G) {
                vf4 xv[U], gv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int v = v0 + u * G;
                    if (v < nvec) {
                        xv[u] = ld16u<NT>(xr + 4 * v);
                        gv[u] = ld16u<NT>(gr + 4 * v);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int v = v0 + u * G;
                    if (v >= nvec) break;
                    vf4 o;
                    o.x = igrad_elem<SUMS>(xv[u].x, gv[u].x, k, q.lo, q.hi, sa, sb);
                    o.y = igrad_elem<SUMS>(xv[u].y, gv[u].y, k, q.lo, q.hi, sa, sb);
                    o.z = igrad_elem<SUMS>(xv[u].z, gv[u].z, k, q.lo, q.hi, sa, sb);
                    o.w = igrad_elem<SUMS>(xv[u].w, gv[u].w, k, q.lo, q.hi, sa, sb);
                    if (or_) st16u<NT>(or_ + 4 * v, o);
                }
            }
            for (int t = (nvec << 2) + sub; t < inner; t += G) {
                const float o = igrad_elem<SUMS>(xr[t], gr[t], k, q.lo, q.hi, sa, sb);
                if (or_) or_[t] = o;
            }
        }
        if (SUMS) {
            for (int off = G >> 1; off >= 1; off >>= 1) {         // the G lanes of a row are neighbours in one wave
                sa += __shfl_xor(sa, off, 64);
                sb += __shfl_xor(sb, off, 64);
            }
            if (live && sub == 0) igrad_store(sa, sb, row, a, q, gdelta, gzero);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// second launch: block r adds row r's split partials in index order; what was read is zeroed again
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_igrad_final(double *part_a, double *part_b, int nsplit, IGradArgs a, float *gdelta, float *gzero)
{
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    double sa = 0.0, sb = 0.0;
    for (int i = tid; i < nsplit; i += kBlock) {
        if (part_a) {
            sa += part_a[row * nsplit + i];
            part_a[row * nsplit + i] = 0.0;
        }
        if (part_b) {
            sb += part_b[row * nsplit + i];
            part_b[row * nsplit + i] = 0.0;
        }
    }
    block_sum2(sa, sb);
    if (tid == 0) igrad_store(sa, sb, row, a, igrad_grid(a), gdelta, gzero);
}

}  // namespace

extern "C" {

size_t fp8q_int_quantize_bwd_workspace_bytes(int64_t C, int64_t inner, int64_t n_delta)
{
    if (C <= 0 || inner <= 0 || (n_delta != 1 && n_delta != C)) return 0;
    return (size_t)bwd_items_bound(C, inner, n_delta) * 2 * sizeof(double);
}

int fp8q_int_quantize_bwd_f32(const float *x, const float *g, float *gx, int64_t C, int64_t inner, const float *delta,
                              const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                              int symmetric, float eps, int64_t grad_scale_elems, float *gdelta, float *gzero_float, void *ws,
                              size_t ws_bytes, fp8q_stream_t stream)
{
    if (!x || !g || !delta || C <= 0 || inner <= 0 || (n_delta != 1 && n_delta != C)) return FP8Q_EINVAL;
    if (symmetric ? !signed_flag : !zero_float) return FP8Q_EINVAL;
    if (!gx && !gdelta && !gzero_float) return FP8Q_EINVAL;
    if (gzero_float && symmetric) return FP8Q_EINVAL;
    if (grad_scale_elems < 0) return FP8Q_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)g | (uintptr_t)gx | (uintptr_t)delta | (uintptr_t)zero_float | (uintptr_t)gdelta |
          (uintptr_t)gzero_float) & 3) != 0)
        return FP8Q_EINVAL;
    if (C > ((int64_t)1 << 42) / inner) return FP8Q_EINVAL;
    IGradArgs a = {};
    if (int rc = make_int_grid(n_bits, a.grid)) return rc;
    const bool sums = gdelta || gzero_float;
    const BwdPlan p = bwd_plan(C, inner, n_delta);
    if (p.blocks > 0x7fffffffll) return FP8Q_EINVAL;
    if (sums && (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < fp8q_int_quantize_bwd_workspace_bytes(C, inner, n_delta)))
        return FP8Q_EWORKSPACE;
    if (sums && (size_t)p.blocks * 2 * sizeof(double) > ws_bytes) return FP8Q_EWORKSPACE;   // (the plan never exceeds its bound)

    a.delta = delta;
    a.zf = symmetric ? nullptr : zero_float;
    a.sflag = signed_flag;
    a.symmetric = symmetric != 0;
    a.scaled = grad_scale_elems > 0;
    a.eps = eps;
    if (a.scaled) {
        a.gs_u = (float)(1.0 / sqrt((double)a.grid.n_hi_u * (double)grad_scale_elems));
        a.gs_s = (float)(1.0 / sqrt((double)a.grid.n_hi_s * (double)grad_scale_elems));
    }

    hipStream_t st = (hipStream_t)stream;
    const bool split_rows = !p.shortrows && p.nsplit > 1;
    double *part_a = (gdelta && split_rows) ? (double *)ws : nullptr;
    double *part_b = (gzero_float && split_rows) ? (double *)ws + p.blocks : nullptr;
    const dim3 grid((unsigned)p.blocks), block(kBlock);
    if (p.shortrows) {
#define FP8Q_IGRAD_SHORT(N, S)                                                                                         \
    hipLaunchKernelGGL((k_igrad_short<N, S>), grid, block, 0, st, x, g, gx, p.C, (int)p.inner, p.G, a, gdelta, gzero_float)
        if (sums) {
            if (p.nt) FP8Q_IGRAD_SHORT(true, true);
            else FP8Q_IGRAD_SHORT(false, true);
        } else {
            if (p.nt) FP8Q_IGRAD_SHORT(true, false);
            else FP8Q_IGRAD_SHORT(false, false);
        }
#undef FP8Q_IGRAD_SHORT
    } else {
#define FP8Q_IGRAD_ROWS(N, UU, S)                                                                                      \
    hipLaunchKernelGGL((k_igrad_rows<N, UU, S>), grid, block, 0, st, x, g, gx, p.inner, (int)p.nsplit, a, gdelta, gzero_float, \
                       part_a, part_b)
        if (sums) {
            if (p.nt) FP8Q_IGRAD_ROWS(true, kUnroll, true);
            else if (p.U == 1) FP8Q_IGRAD_ROWS(false, 1, true);
            else FP8Q_IGRAD_ROWS(false, kUnroll, true);
        } else {
            if (p.nt) FP8Q_IGRAD_ROWS(true, kUnroll, false);
            else if (p.U == 1) FP8Q_IGRAD_ROWS(false, 1, false);
            else FP8Q_IGRAD_ROWS(false, kUnroll, false);
        }
#undef FP8Q_IGRAD_ROWS
    }
    if (int rc = launch_rc()) return rc;
    if (part_a || part_b) {
        hipLaunchKernelGGL(k_igrad_final, dim3((unsigned)p.C), block, 0, st, part_a, part_b, (int)p.nsplit, a, gdelta,
                           gzero_float);
        return launch_rc();
    }
    return FP8Q_OK;
}

}  // extern "C"
