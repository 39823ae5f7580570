// fp8q_grad.hip -- backward of the FP8 fake-quantizer (quantize_to_fp8_ste_MM, fp8_quantizer.py:105-133) in one
// streaming pass: d/dx, d/dmaxval and d/dmbits from x and the upstream gradient g (include/fp8q.h: fp8q_quantize_bwd_f32).
//
// Per element, in fp32 and in the order the autograd chain of quantization/fp8.py:_FakeQuantSTE forms it
// (lo = -maxval for a signed format, 0 for an unsigned one; y = the forward's result, RECOMPUTED here with the forward's own
// per-element code of fp8q_device.h, so nobody has to keep y between the forward and the backward):
//     m  = [lo < x < maxval] + 0.5 [x == maxval or x == lo]                    gx = g * m
//     xc = min(max(x, lo), maxval),  d = y - xc
//     w  = ((d / maxval + [x > maxval]) + 0.5 [x == maxval]) (- [x < lo]) (- 0.5 [x == lo])     (the last two: signed only)
//     gmaxval[row] = sum g * w,     gmbits = ln2 (-1 - bias'(M)) sum g * d
// The products g * w and g * d are fp32, the sums fp64.  A NaN x gives gx = 0 (every comparison is false) and NaN sums
// (y is NaN).
//
// The reductions are deterministic: every lane adds its elements in a fixed order, lanes and waves are combined by a fixed
// tree, blocks by a second small launch that adds the per-block partial sums (8-byte words of the caller's workspace) in index
// order.  No floating-point atomics, no spinning: the kernel boundary hands the partials over.  The finalising launch
// zeroes every word it has read, so the workspace is left as it was found.
//
//   k_bwd_rows    per tensor, and per-channel rows longer than kShortMaxInner: a block = (row, split); a row's table
//                 in LDS as in k_quant_rows; split s streams the 16 KiB pieces s, s + nsplit, ... of its row.
//   k_bwd_short   per-channel rows up to kShortMaxInner elements: G lanes own a row (G a power of two <= 64), kBlock / G
//                 rows per pass; the row's sum never leaves the wave and gmaxval[row] is written at once.
//   k_bwd_final   block r < rows: gmaxval[r] = sum of row r's split partials; one more block: gmbits.
// All accesses are 16 bytes per lane at 4-byte alignment (rows start anywhere; x, g and gx need not share a phase).
#include "fp8q_common.h"
#include "fp8q_bwd.h"

namespace {

// The format: by value (mbits_dev == nullptr: tab[0]), or every width the call admits when the width is a device scalar
struct BwdFmt {
    const float *mbits_dev;
    int hi;          // n_bits - sign_bits
    int lut_stride;  // entries per table row in LDS: the largest pmax + 1 among the admitted formats
    QFmt tab[8];     // tab[M - 1]
};

__device__ __forceinline__ QFmt bwd_pick(const BwdFmt &s)
{
    if (!s.mbits_dev) return s.tab[0];
    float M = rintf(*s.mbits_dev);                       // torch.round: half to even (fp8_quantizer.py:105)
    M = fminf(fmaxf(M, 1.0f), (float)s.hi);              // (NaN -> 1, as fp8q_quantize_dm_f32)
    return s.tab[(int)M - 1];
}

// one element: returns gx, adds its terms to the two sums
template <bool SUMS>
__device__ __forceinline__ float bwd_elem(float x, float y, float g, float maxv, float lo, int sgn, double &sa, double &sb)
{
    const bool at_hi = x == maxv, at_lo = x == lo;
    const float m = (((x > lo) & (x < maxv)) ? 1.0f : 0.0f) + 0.5f * ((at_hi | at_lo) ? 1.0f : 0.0f);
    if (SUMS) {
        const float xc = fminf(fmaxf(x, lo), maxv);     // (a NaN x: y is NaN, so d is NaN whatever xc is)
        const float d = y - xc;
        float w = d / maxv;
        w = w + (x > maxv ? 1.0f : 0.0f);
        w = w + 0.5f * (at_hi ? 1.0f : 0.0f);
        if (sgn) {
            w = w - (x < lo ? 1.0f : 0.0f);
            w = w - 0.5f * (at_lo ? 1.0f : 0.0f);
        }
        sa += (double)(g * w);
        sb += (double)(g * d);
    }
    return g * m;
}

// the forward of N elements of one channel
template <int N, bool LUT>
__device__ __forceinline__ void fwd_group(const float (&x)[N], float (&y)[N], const Chan &cf, const ChanLite &c,
                                          const float2 *lut, const QFmt &f)
{
    if (LUT) {
#pragma unroll
        for (int j = 0; j < N; ++j) y[j] = x[j];
        quant_group<N>(y, c, lut, (float)f.pmax, f.qthr);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) y[j] = quant_direct(x[j], cf, f.M);
    }
}

// ---------------------------------------------------------------------------------------------
// long rows: block = (row, split)
// ---------------------------------------------------------------------------------------------
template <bool NT, int U, bool SUMS>
__global__ void __launch_bounds__(kBlock)
k_bwd_rows(const float *__restrict__ x, const float *__restrict__ g, float *__restrict__ gx, int64_t inner, int nsplit,
           const float *__restrict__ maxval, int per_channel, BwdFmt bf, float *gmaxval, double *part_a, double *part_b)
{
    __shared__ float2 lut[kLutMax];
    const QFmt f = bwd_pick(bf);
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x / (unsigned)nsplit;
    const int split = (int)(blockIdx.x - row * nsplit);
    const float maxv = maxval[per_channel ? row : 0];
    Chan cfull;
    ChanLite c;
    if (SUMS) {
        cfull = make_chan(maxv, f);
        for (int i = tid; i <= f.pmax; i += kBlock) lut[i] = lut_entry(cfull, i, f.M);
        __syncthreads();
        c = lite(cfull);
    }
    const float lo = f.sign_bits == 1 ? -maxv : 0.0f;
    const int sgn = f.sign_bits;
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
            float xe[U * 4], ge[U * 4], ye[U * 4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                xe[4 * u + 0] = xv[u].x, xe[4 * u + 1] = xv[u].y, xe[4 * u + 2] = xv[u].z, xe[4 * u + 3] = xv[u].w;
                ge[4 * u + 0] = gv[u].x, ge[4 * u + 1] = gv[u].y, ge[4 * u + 2] = gv[u].z, ge[4 * u + 3] = gv[u].w;
            }
            if (SUMS) fwd_group<U * 4, true>(xe, ye, cfull, c, lut, f);
#pragma unroll
            for (int j = 0; j < U * 4; ++j) ge[j] = bwd_elem<SUMS>(xe[j], SUMS ? ye[j] : 0.0f, ge[j], maxv, lo, sgn, sa, sb);
            if (or_) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    st16u<NT>(or_ + 4 * (base + u * kBlock + tid), vf4{ge[4 * u + 0], ge[4 * u + 1], ge[4 * u + 2], ge[4 * u + 3]});
            }
        } else {
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + u * kBlock + tid;
                if (i < nvec) {
                    const vf4 xv = ld16u<NT>(xr + 4 * i), gv = ld16u<NT>(gr + 4 * i);
                    const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
                    float ge[4] = {gv.x, gv.y, gv.z, gv.w}, ye[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (SUMS) fwd_group<4, true>(xe, ye, cfull, c, lut, f);
#pragma unroll
                    for (int j = 0; j < 4; ++j) ge[j] = bwd_elem<SUMS>(xe[j], ye[j], ge[j], maxv, lo, sgn, sa, sb);
                    if (or_) st16u<NT>(or_ + 4 * i, vf4{ge[0], ge[1], ge[2], ge[3]});
                }
            }
        }
    }
    if (split == 0) {                         // the <= 3 elements behind the last 16-byte group of the row
        const int64_t t = (nvec << 2) + tid;
        if (t < inner) {
            const float xe = xr[t];
            const float ye = SUMS ? quant_one(xe, c, lut, (float)f.pmax, f.qthr) : 0.0f;
            const float o = bwd_elem<SUMS>(xe, ye, gr[t], maxv, lo, sgn, sa, sb);
            if (or_) or_[t] = o;
        }
    }
    if (SUMS) {
        block_sum2(sa, sb);
        if (tid == 0) {
            if (gmaxval && nsplit == 1) gmaxval[row] = (float)sa;
            else if (part_a) part_a[blockIdx.x] = sa;
            if (part_b) part_b[blockIdx.x] = sb;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// short rows: G lanes own a row
// ---------------------------------------------------------------------------------------------
template <bool NT, bool SUMS, bool LUT>
__global__ void __launch_bounds__(kBlock)
k_bwd_short(const float *__restrict__ x, const float *__restrict__ g, float *__restrict__ gx, int64_t C, int inner, int G,
            const float *__restrict__ maxval, BwdFmt bf, float *gmaxval, double *part_b)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const QFmt f = bwd_pick(bf);
    const int tid = threadIdx.x;
    const int sub = tid & (G - 1), slot = tid / G, rpp = kBlock / G;
    float2 *lut = reinterpret_cast<float2 *>(smem) + (LUT ? slot * bf.lut_stride : 0);
    const int sgn = f.sign_bits;
    const int nvec = inner >> 2;
    const int64_t npass = (C + rpp - 1) / rpp;
    double sb_all = 0.0;
    for (int64_t p = blockIdx.x; p < npass; p += gridDim.x) {     // (uniform over the block: barriers inside)
        const int64_t row = p * rpp + slot;
        const bool live = row < C;
        const float maxv = live ? maxval[row] : 1.0f;
        const float lo = sgn == 1 ? -maxv : 0.0f;
        Chan cfull;
        ChanLite c;
        if (SUMS) {
            if (LUT) __syncthreads();         // the previous pass no longer reads its tables
            cfull = make_chan(maxv, f);
            if (LUT) {
                lut_part(lut, cfull, f, sub, G);
                __syncthreads();
            }
            c = lite(cfull);
        }
        double sa = 0.0, sb = 0.0;
        if (live) {
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
                    const float xe[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
                    float ge[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w}, ye[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (SUMS) fwd_group<4, LUT>(xe, ye, cfull, c, lut, f);
#pragma unroll
                    for (int j = 0; j < 4; ++j) ge[j] = bwd_elem<SUMS>(xe[j], ye[j], ge[j], maxv, lo, sgn, sa, sb);
                    if (or_) st16u<NT>(or_ + 4 * v, vf4{ge[0], ge[1], ge[2], ge[3]});
                }
            }
            for (int t = (nvec << 2) + sub; t < inner; t += G) {
                const float xe[1] = {xr[t]};
                float ye[1] = {0.0f};
                if (SUMS) fwd_group<1, LUT>(xe, ye, cfull, c, lut, f);
                const float o = bwd_elem<SUMS>(xe[0], ye[0], gr[t], maxv, lo, sgn, sa, sb);
                if (or_) or_[t] = o;
            }
        }
        if (SUMS) {
            for (int off = G >> 1; off >= 1; off >>= 1) {         // the G lanes of a row are neighbours in one wave
                sa += __shfl_xor(sa, off, 64);
                sb += __shfl_xor(sb, off, 64);
            }
            if (live && sub == 0) {
                if (gmaxval) gmaxval[row] = (float)sa;
                sb_all += sb;
            }
        }
    }
    if (SUMS && part_b) {
        double dummy = 0.0;
        block_sum2(sb_all, dummy);
        if (tid == 0) part_b[blockIdx.x] = sb_all;
    }
}

// ---------------------------------------------------------------------------------------------
// second launch: partial sums -> gmaxval / gmbits, in index order; what was read is zeroed again
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_bwd_final(double *part_a, int nsplit, int rows_a, float *gmaxval, double *part_b, int64_t n_b, float *gmbits, float mbits,
            const float *mbits_dev, int hi)
{
    const int tid = threadIdx.x;
    double s = 0.0, dummy = 0.0;
    if ((int)blockIdx.x < rows_a) {
        double *p = part_a + (int64_t)blockIdx.x * nsplit;
        for (int i = tid; i < nsplit; i += kBlock) {
            s += p[i];
            p[i] = 0.0;
        }
        block_sum2(s, dummy);
        if (tid == 0) gmaxval[blockIdx.x] = (float)s;
        return;
    }
    for (int64_t i = tid; i < n_b; i += kBlock) {
        s += part_b[i];
        part_b[i] = 0.0;
    }
    block_sum2(s, dummy);
    if (tid == 0) {
        // M = clamp(round_ste(mbits), 1, hi): round_ste passes the gradient, the clamp cuts it off outside [1, hi]
        const double r = (double)rintf(mbits_dev ? *mbits_dev : mbits);
        float out = 0.0f;
        if (r >= 1.0 && r <= (double)hi) {
            const double ln2 = 0.69314718055994530942;
            const double two_mM = ldexp(1.0, -(int)r);
            const double dbias = -ln2 * ldexp(1.0, hi - (int)r) + two_mM / (2.0 - two_mM);
            out = (float)(s * (ln2 * (-1.0 - dbias)));
        }
        gmbits[0] = out;
    }
}

}  // namespace

extern "C" {

size_t fp8q_quantize_bwd_workspace_bytes(int64_t C, int64_t inner, int64_t n_maxval)
{
    if (C <= 0 || inner <= 0 || (n_maxval != 1 && n_maxval != C)) return 0;
    return (size_t)bwd_items_bound(C, inner, n_maxval) * 2 * sizeof(double);
}

int fp8q_quantize_bwd_f32(const float *x, const float *g, float *gx, int64_t C, int64_t inner, const float *maxval,
                          int64_t n_maxval, float mbits, const float *mbits_dev, int n_bits, int sign_bits, float *gmaxval,
                          float *gmbits, void *ws, size_t ws_bytes, fp8q_stream_t stream)
{
    if (!x || !g || !maxval || C <= 0 || inner <= 0 || (n_maxval != 1 && n_maxval != C)) return FP8Q_EINVAL;
    if (sign_bits != 0 && sign_bits != 1) return FP8Q_EINVAL;
    if (!gx && !gmaxval && !gmbits) return FP8Q_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)g | (uintptr_t)gx | (uintptr_t)maxval | (uintptr_t)mbits_dev | (uintptr_t)gmaxval |
          (uintptr_t)gmbits) & 3) != 0)
        return FP8Q_EINVAL;
    if (C > ((int64_t)1 << 42) / inner) return FP8Q_EINVAL;
    BwdFmt bf = {};
    bf.mbits_dev = mbits_dev;
    bf.hi = n_bits - sign_bits;
    if (mbits_dev) {
        if (n_bits < 2 || n_bits > 16) return FP8Q_EINVAL;
        if (bf.hi > 8) return FP8Q_EUNSUPPORTED;     // the narrowest width would need more than 7 exponent bits
        for (int M = 1; M <= 8; ++M)
            if (int rc = make_fmt((float)(M <= bf.hi ? M : bf.hi), n_bits, sign_bits, &bf.tab[M - 1])) return rc;
        bf.lut_stride = bf.tab[0].pmax + 1;
    } else {
        if (int rc = make_fmt(mbits, n_bits, sign_bits, &bf.tab[0])) return rc;
        for (int i = 1; i < 8; ++i) bf.tab[i] = bf.tab[0];
        bf.lut_stride = bf.tab[0].pmax + 1;
    }
    const bool sums = gmaxval || gmbits;
    const BwdPlan p = bwd_plan(C, inner, n_maxval);
    if (p.blocks > 0x7fffffffll) return FP8Q_EINVAL;
    if (sums && (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < fp8q_quantize_bwd_workspace_bytes(C, inner, n_maxval)))
        return FP8Q_EWORKSPACE;
    if (sums && (size_t)p.blocks * 2 * sizeof(double) > ws_bytes) return FP8Q_EWORKSPACE;   // (the plan never exceeds its bound)

    hipStream_t st = (hipStream_t)stream;
    double *part_a = nullptr, *part_b = nullptr;
    const bool split_rows = !p.shortrows && p.nsplit > 1;
    if (gmaxval && split_rows) part_a = (double *)ws;
    if (gmbits) part_b = (double *)ws + p.blocks;
    const dim3 grid((unsigned)p.blocks), block(kBlock);
    if (p.shortrows) {
        const bool lut = sums && p.inner >= 2 * (int64_t)bf.lut_stride;
        const size_t shmem = lut ? (size_t)(kBlock / p.G) * bf.lut_stride * sizeof(float2) : 0;
#define FP8Q_BWD_SHORT(N, S, L)                                                                                        \
    hipLaunchKernelGGL((k_bwd_short<N, S, L>), grid, block, shmem, st, x, g, gx, p.C, (int)p.inner, p.G, maxval, bf, gmaxval, \
                       part_b)
        if (!sums) {
            if (p.nt) FP8Q_BWD_SHORT(true, false, false);
            else FP8Q_BWD_SHORT(false, false, false);
        } else if (lut) {
            if (p.nt) FP8Q_BWD_SHORT(true, true, true);
            else FP8Q_BWD_SHORT(false, true, true);
        } else {
            if (p.nt) FP8Q_BWD_SHORT(true, true, false);
            else FP8Q_BWD_SHORT(false, true, false);
        }
#undef FP8Q_BWD_SHORT
    } else {
        const int pc = n_maxval != 1;
#define FP8Q_BWD_ROWS(N, UU, S)                                                                                        \
    hipLaunchKernelGGL((k_bwd_rows<N, UU, S>), grid, block, 0, st, x, g, gx, p.inner, (int)p.nsplit, maxval, pc, bf, gmaxval, \
                       part_a, part_b)
        if (sums) {
            if (p.nt) FP8Q_BWD_ROWS(true, kUnroll, true);
            else if (p.U == 1) FP8Q_BWD_ROWS(false, 1, true);
            else FP8Q_BWD_ROWS(false, kUnroll, true);
        } else {
            if (p.nt) FP8Q_BWD_ROWS(true, kUnroll, false);
            else if (p.U == 1) FP8Q_BWD_ROWS(false, 1, false);
            else FP8Q_BWD_ROWS(false, kUnroll, false);
        }
#undef FP8Q_BWD_ROWS
    }
    if (int rc = launch_rc()) return rc;
    if (part_a || part_b) {
        const int rows_a = part_a ? (int)p.C : 0;
        hipLaunchKernelGGL(k_bwd_final, dim3((unsigned)(rows_a + (part_b ? 1 : 0))), block, 0, st, part_a, (int)p.nsplit, rows_a,
                           gmaxval, part_b, p.blocks, gmbits, mbits, mbits_dev, bf.hi);
        return launch_rc();
    }
    return FP8Q_OK;
}

}  // extern "C"
