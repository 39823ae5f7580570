// fp8q_int.hip -- uniform (INT) fake-quantization on gfx950: the reference's SymmetricUniformQuantizer /
// AsymmetricUniformQuantizer (uniform_quantizers.py) with linear scale domain, and their range setting.
//
// Arithmetic contract (bit for bit the reference's fp32 op chain, every op rounded on its own; -ffp-contract=off):
//   range       xmin' = min(xmin, 0),  xmax' = max(xmax, eps)                      (_tensorize_min_max)
//               asymmetric: delta = (xmax' - xmin') / int_max,  zero_float = -xmin' / delta
//               symmetric:  signed = (min over ALL channels of xmin') < 0     -- one flag per quantizer; a NaN
//                           anywhere makes it false (torch.min propagates NaN, NaN < 0 is false)
//                           delta = max(|xmin'|, xmax') / int_max(signed)
//   quantize    scale = max(delta, eps)
//               zp = clamp(rint(zero_float), int_min, int_max)  (asymmetric),  0 (symmetric)
//               y  = scale * (clamp(rint(x / scale) + zp, int_min, int_max) - zp)
//               [int_min, int_max] = [-2^(n-1), 2^(n-1) - 1] when signed, [0, 2^n - 1] otherwise (asymmetric:
//               unsigned); the symmetric sign is read from device memory -- no host round trip.
//   min / max / clamp propagate NaN as torch's do (a bare fminf / fmaxf would not); +-inf saturates to the clamp
//   ends.  min(xmin, 0) keeps an xmin of -0 (torch's scalar loop: per-tensor ranges; torch's vectorised CPU loop
//   returns the +0 operand -- the one case where the two torch paths themselves differ).  rint rounds half to even.
//
// x / scale without a division per element: r = fl32(1 / scale) once per channel (IEEE division), q0 = fl32(x * r).
// |q0 - x/scale| <= |x/scale| (2^-24 + 2^-24 + 2^-48) and |fl32(x/scale) - x/scale| <= 2^-24 |x/scale|, so q0 and
// fl32(x / scale) differ by less than 2^-22 |q0| (1 + 2^-22).  rint(q0) == rint(fl32(x / scale)) unless q0 lies
// within that distance of a rounding tie: lanes with |q0 - rint(q0)| >= 0.5 - 2^-20 |q0| redo the IEEE division
// (4x margin; a tie itself is always redone).  Subnormal quotients have |q| < 0.5 and round to a zero of x's sign on
// both paths; an overflow to inf on one path only happens at |q| > 2^127, where both clamp to int_max / int_min; NaN
// fails the comparison and stays NaN.
//
// Kernels:
//   k_int_quant<RANGE, PC, VEC, NT>  one aligned 4096-element chunk per block (K1's streaming: 16 B per lane per
//                 access, 4 accesses in flight, neighbouring blocks on neighbouring chunks).  The channel constants
//                 {scale, 1/scale, zp} of the rows overlapping the chunk are built once per block in LDS, from
//                 (delta, zero_float) -- or, RANGE, from (xmin, xmax), with the block in which a row starts writing
//                 that row's delta / zero_float (and block 0 the sign): range-set and quantize in one launch.
//                 The kernel is fp8q_intq.h's chunk_setup() + chunk_walk() with int_one as the element's operation;
//                 the integer grid, the argument block, the sign and the launch's host side live there too.
//   k_int_sign    the global sign of a symmetric per-channel range with more than kSignInline channels (fewer: every
//                 block of k_int_quant / k_int_range folds it itself from the xmin vector).
//   k_int_range   range-set alone: (xmin, xmax) -> delta, zero_float, signed.
//   k_int_sse<T>  the line search's candidates in one pass (see "The candidate search" below), k_int_sse_final its sums.
#include "fp8q_common.h"
#include "fp8q_intq.h"

namespace {

// ---------------------------------------------------------------------------------------------
// The candidate search (LineSearchEstimator with a uniform quantizer): out[k, c] += sum over row c of (x - q_k(x))^2,
// q_k the quantizer after set_quant_range(one_sided ? 0 : -thr[k, c], thr[k, c]) -- range_of / consts_of (fp8q_intq.h) on a
// one-element range, the symmetric sign being that element's (x_min < 0; a NaN threshold: unsigned).
//   float32 x: int_one, then d = x - y and d * d in fp32 (the reference's chain on a float32 sample), widened exactly.
//   float64 x: ATen's promotion with a float64 tensor and 0-dim fp32 scale / zero point: both widened exactly, every op
//              from the division to the square in double.  x / scale as in int_one: q0 = fl64(x * r), r = fl64(1 / scale)
//              once per candidate; |q0 - x/scale| <= |x/scale| (2^-52 + 2^-106) and |fl64(x/scale) - x/scale| <=
//              2^-53 |x/scale|, so the two differ by less than 2^-51 |q0|: lanes with |q0 - rint(q0)| >= 0.5 - 2^-50 |q0|
//              (2x margin; a tie itself, and everything from 2^49 up, is redone) take the IEEE division.  scale >= eps
//              is a float32 value, so r is a normal double or, for scale = 0 / inf / NaN, what makes x * r agree with x /
//              scale in kind (inf, 0, NaN); an overflow of x * r alone needs |x| > 1e300, where both quotients clamp to
//              the same end; subnormal quotients round to a zero of x's sign on both paths.
// Layout (k_sse_f64's, fp8q_f64.hip): lane = candidate.  A block owns 256 candidates of one row and walks its share of
// the row in tiles of 1024 elements staged in LDS; every lane reads the SAME element (LDS broadcast), quantizes it for
// its own candidate and adds the square to a register: no cross-lane reduction, candidate constants in registers.
// 32 squares go into a short accumulator, short accumulators into the block's (all float64): any order of n
// non-negative terms is within (n - 1) 2^-53 of their exact sum, this one within ~(32 + tiles * 32) 2^-53.
// Partials ws[c][split][cand] are fully written (no initialisation needed); k_int_sse_final adds the splits of a
// candidate in a fixed order -- 8 interleaved running sums, then those 8 in order -- and accumulates into out: no
// floating-point atomics, the same bits on every call.
// ---------------------------------------------------------------------------------------------
constexpr int kIntSseTile = 1024;
constexpr int kIntSseMaxCand = 1 << 20;

__device__ __forceinline__ double t_clamp(double v, double lo, double hi)
{
    return (v != v) ? v : (v < lo ? lo : (v > hi ? hi : v));
}

struct IntCand {
    float4 k;        // consts_of: {scale, 1/scale, zp, -}
    float lo, hi;
    double s, r, zp; // float64 lane: scale and zp widened, r = 1 / scale in double
};

__device__ __forceinline__ IntCand int_cand(float thr, bool symmetric, bool one_sided, float eps, const IntGrid &grid)
{
    const float xmin = one_sided ? 0.0f : -thr;
    const bool sgn = symmetric && xmin < 0.0f;
    IntCand c;
    c.lo = grid.lo(sgn);
    c.hi = grid.hi(sgn);
    const Range r = range_of(xmin, thr, symmetric, c.hi, eps);
    c.k = consts_of(r.delta, r.zf, symmetric, c.lo, c.hi, eps);
    c.s = (double)c.k.x;
    c.r = 1.0 / c.s;
    c.zp = (double)c.k.z;
    return c;
}

// (x - q(x))^2 of one element, as a double
__device__ __forceinline__ double int_sq(float v, const IntCand &c)
{
    const float d = v - int_one(v, c.k, c.lo, c.hi);
    return (double)(d * d);
}
__device__ __forceinline__ double int_sq(double v, const IntCand &c)
{
    const double q0 = v * c.r;
    double rq = rint(q0);
    if (fabs(q0 - rq) >= 0.5 - fabs(q0) * 0x1p-50) rq = rint(v / c.s);
    const double t = t_clamp(rq + c.zp, (double)c.lo, (double)c.hi);
    const double d = v - c.s * (t - c.zp);
    return d * d;
}

struct IntSseArgs {
    int64_t C, inner, ntiles;
    int n_cand, nsplit, tpb;
    int symmetric, one_sided;
    float eps;
    IntGrid grid;
};

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_int_sse(const T *__restrict__ x, const float *__restrict__ thr, double *__restrict__ ws, IntSseArgs a)
{
    __shared__ __attribute__((aligned(16))) T xs[kIntSseTile];
    const int tid = threadIdx.x;
    const int split = blockIdx.x;
    const int cand = blockIdx.y * kBlock + tid;
    const int64_t c = blockIdx.z;
    const bool active = cand < a.n_cand;
    const float tv = active ? thr[(int64_t)cand * a.C + c] : 1.0f;
    const IntCand ch = int_cand(tv, a.symmetric != 0, a.one_sided != 0, a.eps, a.grid);
    const T *xr = x + c * a.inner;
    double acc = 0.0;
    const int64_t t_begin = (int64_t)split * a.tpb;
    const int64_t t_end = t_begin + a.tpb < a.ntiles ? t_begin + a.tpb : a.ntiles;
    for (int64_t t = t_begin; t < t_end; ++t) {
        const int64_t e0 = t * kIntSseTile;
        const int n = (int)(a.inner - e0 < kIntSseTile ? a.inner - e0 : kIntSseTile);
        __syncthreads();
        for (int i = tid; i < n; i += kBlock) xs[i] = xr[e0 + i];
        __syncthreads();
        const int n32 = n & ~31;
        for (int j = 0; j < n32; j += 32) {
            double pa = 0.0;
#pragma unroll 8
            for (int u = 0; u < 32; ++u) pa += int_sq(xs[j + u], ch);
            acc += pa;
        }
        if (n32 < n) {
            double pa = 0.0;
            for (int j = n32; j < n; ++j) pa += int_sq(xs[j], ch);
            acc += pa;
        }
    }
    if (active) ws[(c * a.nsplit + split) * a.n_cand + cand] = acc;
}

// out[k, c] += the splits' partials: 32 candidates x 8 interleaved running sums per block, combined in order
__global__ void __launch_bounds__(kBlock)
k_int_sse_final(const double *__restrict__ ws, double *__restrict__ out, int64_t C, int n_cand, int nsplit)
{
    __shared__ double part[8][32];
    const int l = threadIdx.x & 31, p = threadIdx.x >> 5;
    const int cand = blockIdx.x * 32 + l;
    const int64_t c = blockIdx.y;
    double sum = 0.0;
    if (cand < n_cand)
        for (int s2 = p; s2 < nsplit; s2 += 8) sum += ws[(c * nsplit + s2) * n_cand + cand];
    part[p][l] = sum;
    __syncthreads();
    if (p == 0 && cand < n_cand) {
        double tot = part[0][l];
#pragma unroll
        for (int q = 1; q < 8; ++q) tot += part[q][l];
        out[(int64_t)cand * C + c] += tot;
    }
}

template <bool RANGE, bool PC, bool VEC, bool NT>
__global__ void __launch_bounds__(kBlock)
k_int_quant(const float *__restrict__ x, float *__restrict__ y, IntArgs a)
{
    extern __shared__ float4 kc[];    // nc_max channel constants
    // RANGE: a row's range from (x_min, x_max); the block in whose chunk the row starts reports it
    auto range = [&](int64_t row, bool starts, float hi) -> Range {
        return RANGE ? SetRange{a}(row, starts, hi) : ReadRange{a}(row, starts, hi);
    };
    const Chunk c = chunk_setup<PC>(a, kc, range, RANGE && a.sign_inline);
    chunk_walk<PC, VEC, NT, int_one>(x, y, c);
}

__global__ void __launch_bounds__(1024) k_int_sign(const float *__restrict__ xmin, int64_t C, unsigned char *sflag)
{
    const bool sgn = block_sign(xmin, C);
    if (threadIdx.x == 0) sflag[0] = (unsigned char)sgn;
}

__global__ void __launch_bounds__(kBlock) k_int_range(IntArgs a)
{
    const float hi = a.grid.hi(int_sign(a, a.sign_inline != 0, a.C > 1));
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < a.C; c += (int64_t)gridDim.x * kBlock) {
        const Range r = range_of(a.a[c], a.b[c], a.symmetric, hi, a.eps);
        a.delta_out[c] = r.delta;
        if (!a.symmetric) a.zf_out[c] = r.zf;
    }
}

struct IntSseGeo {
    int64_t ntiles;
    int nsplit, tpb, cgroups;
};

// splits of a row: up to 2 x kTargetBlocks / C, equal shares of tiles.  Independent of n_cand (so the workspace grows with
// it), and a search with few candidates still fills the chip.
IntSseGeo int_sse_geo(int64_t C, int64_t inner, int64_t n_cand)
{
    IntSseGeo g;
    g.ntiles = cdiv(inner, kIntSseTile);
    g.cgroups = (int)cdiv(n_cand, kBlock);
    const int64_t nsplit = balanced_blocks(g.ntiles, 2 * (int64_t)kTargetBlocks / C);
    g.tpb = (int)cdiv(g.ntiles, nsplit);
    g.nsplit = (int)cdiv(g.ntiles, g.tpb);
    return g;
}

template <typename T>
int int_sse_grid(const T *x, int64_t C, int64_t inner, const float *thr, int64_t n_cand, int n_bits, int symmetric,
                 int one_sided, float eps, double *out, void *ws, size_t ws_bytes, hipStream_t st)
{
    if (!x || !thr || !out || C <= 0 || inner <= 0 || n_cand <= 0 || n_cand > kIntSseMaxCand ||
        ((uintptr_t)x & (sizeof(T) - 1)) || ((uintptr_t)thr & 3) || ((uintptr_t)out & 7))
        return FP8Q_EINVAL;
    IntSseArgs a;
    if (int rc = make_int_grid(n_bits, a.grid)) return rc;
    if (C > 65535) return FP8Q_ETOOMANY;
    if (inner > INT64_MAX / C) return FP8Q_EINVAL;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < fp8q_int_sse_grid_workspace_bytes(C, inner, n_cand)) return FP8Q_EWORKSPACE;
    const IntSseGeo g = int_sse_geo(C, inner, n_cand);
    a.C = C;
    a.inner = inner;
    a.ntiles = g.ntiles;
    a.n_cand = (int)n_cand;
    a.nsplit = g.nsplit;
    a.tpb = g.tpb;
    a.symmetric = symmetric != 0;
    a.one_sided = one_sided != 0;
    a.eps = eps;
    hipLaunchKernelGGL(k_int_sse<T>, dim3((unsigned)g.nsplit, (unsigned)g.cgroups, (unsigned)C), dim3(kBlock), 0, st, x, thr,
                       (double *)ws, a);
    if (int rc = launch_rc()) return rc;
    hipLaunchKernelGGL(k_int_sse_final, dim3((unsigned)cdiv(n_cand, 32), (unsigned)C), dim3(kBlock), 0, st,
                       (const double *)ws, out, C, (int)n_cand, g.nsplit);
    return launch_rc();
}

// the quantize launch; `range`: a / b are (x_min, x_max) and the launch also writes delta (zero_float, sign)
int int_quant_launch(bool range, const float *x, float *y, int64_t C, int64_t inner, IntArgs a, hipStream_t st)
{
    const bool pc = a.C > 1;
    int_geometry(a, C, inner, pc);
    const bool vec = int_vec16(x, y);
    if (range && pc) FP8Q_INT_LAUNCH(vec, x, y, a, st, k_int_quant, true, true);
    else if (range) FP8Q_INT_LAUNCH(vec, x, y, a, st, k_int_quant, true, false);
    else if (pc) FP8Q_INT_LAUNCH(vec, x, y, a, st, k_int_quant, false, true);
    else FP8Q_INT_LAUNCH(vec, x, y, a, st, k_int_quant, false, false);
    return launch_rc();
}

}  // namespace

int fp8q_int_sign_launch(const float *xmin, int64_t C, unsigned char *sflag, hipStream_t st)
{
    hipLaunchKernelGGL(k_int_sign, dim3(1), dim3(1024), 0, st, xmin, C, sflag);
    return launch_rc();
}

extern "C" {

// What a chunked launch would be made with: the entry points' own steps -- int_check_x, int_geometry, int_sign_inline,
// int_vec16, int_plan (fp8q_intq.h) -- on made-up addresses that have the caller's 16-byte phases and are never
// dereferenced.  Host arithmetic only.
int fp8q_chunk_route(int64_t C, int64_t inner, int64_t n_range, int elem_bytes, int in_mod16, int out_mod16, int symmetric,
                     int sets_range, fp8q_chunk_route_info *info)
{
    if (!info || (elem_bytes != 4 && elem_bytes != 2) || in_mod16 < 0 || in_mod16 > 15 || out_mod16 < 0 || out_mod16 > 15)
        return FP8Q_EINVAL;
    const void *in = reinterpret_cast<const void *>(((uintptr_t)1 << 44) + (uintptr_t)in_mod16);
    const void *out = reinterpret_cast<const void *>(((uintptr_t)1 << 45) + (uintptr_t)out_mod16);
    if (int rc = int_check_x(in, out, C, inner, n_range)) return rc;
    IntArgs a = {};
    a.C = n_range;
    a.symmetric = symmetric != 0;
    const bool pc = a.C > 1;
    int_geometry(a, C, inner, pc);
    const IntPlan p = int_plan(a, int_vec16(in, out), elem_bytes);
    fp8q_chunk_route_info r = {};
    r.per_channel = pc;
    r.rows_per_chunk = a.nc_max;
    r.two_row = pc && a.inner >= kIntChunk;
    r.vec = p.vec;
    r.nontemporal = p.nt;
    r.sign_prepass = sets_range && !int_sign_inline(a.symmetric, a.C);
    r.magic = a.magic;
    r.grid_x = p.grid_x;
    r.lds_bytes = (int64_t)p.lds_bytes;
    r.last_chunk = a.n - (int64_t)(p.grid_x - 1) * kIntChunk;
    *info = r;
    return FP8Q_OK;
}

int fp8q_int_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *delta,
                          const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                          int symmetric, float eps, fp8q_stream_t stream)
{
    if (int rc = int_check_x(x, y, C, inner, n_delta)) return rc;
    IntArgs a = {};
    if (int rc = int_fixed_args(a, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps)) return rc;
    return int_quant_launch(false, x, y, C, inner, a, (hipStream_t)stream);
}

int fp8q_int_set_range_f32(const float *x_min, const float *x_max, int64_t n, float *delta, float *zero_float,
                           unsigned char *signed_flag, int n_bits, int symmetric, float eps, fp8q_stream_t stream)
{
    if (!x_min || !x_max || !delta || n <= 0 || (symmetric ? !signed_flag : !zero_float)) return FP8Q_EINVAL;
    IntArgs a = {};
    if (int rc = make_int_grid(n_bits, a.grid)) return rc;
    a.a = x_min;
    a.b = x_max;
    a.delta_out = delta;
    a.zf_out = zero_float;
    a.sflag = signed_flag;
    a.C = n;
    a.symmetric = symmetric != 0;
    a.eps = eps;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = int_sign_prepass(a, st)) return rc;
    const int64_t nb = cdiv(n, kBlock);
    hipLaunchKernelGGL(k_int_range, dim3((unsigned)(nb < kTargetBlocks ? nb : kTargetBlocks)), dim3(kBlock), 0, st, a);
    return launch_rc();
}

int fp8q_int_range_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *x_min,
                                const float *x_max, int64_t n_range, float *delta, float *zero_float,
                                unsigned char *signed_flag, int n_bits, int symmetric, float eps,
                                fp8q_stream_t stream)
{
    if (int rc = int_check_x(x, y, C, inner, n_range)) return rc;
    if (!x_min || !x_max || !delta || (symmetric ? !signed_flag : !zero_float)) return FP8Q_EINVAL;
    IntArgs a = {};
    if (int rc = make_int_grid(n_bits, a.grid)) return rc;
    a.a = x_min;
    a.b = x_max;
    a.delta_out = delta;
    a.zf_out = zero_float;
    a.sflag = signed_flag;
    a.C = n_range;
    a.symmetric = symmetric != 0;
    a.eps = eps;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = int_sign_prepass(a, st)) return rc;
    return int_quant_launch(true, x, y, C, inner, a, st);
}

int fp8q_int_minmax_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, float *row_min, float *row_max,
                                 float *delta, float *zero_float, unsigned char *signed_flag, int n_bits, int symmetric,
                                 float eps, void *ws, size_t ws_bytes, fp8q_stream_t stream)
{
    if (int rc = int_check_x(x, y, C, inner, C)) return rc;
    if (!row_min || !row_max || !delta || (symmetric ? !signed_flag : !zero_float)) return FP8Q_EINVAL;
    IntGrid probe;
    if (int rc = make_int_grid(n_bits, probe)) return rc;
    if (int rc = fp8q_minmax_f32(x, C, inner, row_min, row_max, nullptr, FP8Q_FOLD_CURRENT, 0.0, 1, ws, ws_bytes,
                                 stream))
        return rc;
    return fp8q_int_range_quantize_f32(x, y, C, inner, row_min, row_max, C, delta, zero_float, signed_flag, n_bits,
                                       symmetric, eps, stream);
}

size_t fp8q_int_sse_grid_workspace_bytes(int64_t C, int64_t inner, int64_t n_cand)
{
    if (C <= 0 || C > 65535 || inner <= 0 || n_cand <= 0 || n_cand > kIntSseMaxCand) return 16;
    return (size_t)C * int_sse_geo(C, inner, n_cand).nsplit * n_cand * sizeof(double) + 16;
}

int fp8q_int_sse_grid_f32(const float *x, int64_t C, int64_t inner, const float *thr, int64_t n_cand, int n_bits,
                          int symmetric, int one_sided, float eps, double *out, void *ws, size_t ws_bytes,
                          fp8q_stream_t stream)
{
    return int_sse_grid(x, C, inner, thr, n_cand, n_bits, symmetric, one_sided, eps, out, ws, ws_bytes, (hipStream_t)stream);
}

int fp8q_int_sse_grid_f64(const double *x, int64_t C, int64_t inner, const float *thr, int64_t n_cand, int n_bits,
                          int symmetric, int one_sided, float eps, double *out, void *ws, size_t ws_bytes,
                          fp8q_stream_t stream)
{
    return int_sse_grid(x, C, inner, thr, n_cand, n_bits, symmetric, one_sided, eps, out, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
