// fp8q_inth16.hip -- the uniform (INT) quantizers on IEEE fp16 and bfloat16 tensors (gfx950 only): fixed ranges, range-set +
// quantize in one launch, and per-channel current_minmax + range + quantize.  Element type selected at run time (x_type /
// y_type = FP8Q_DT_*, include/fp8q.h).
//
// Arithmetic contract:
//   - every input element is widened to fp32 EXACTLY, as fp8q_h16.hip does it (fp8q_half.h): fp16 subnormals become normal
//     fp32 numbers, bf16 is the upper half of an fp32 word, nothing is flushed.
//   - from there the fp32 contract of fp8q_int.hip:4-25 applies unchanged, through the same consts_of / int_level / range_of
//     code (fp8q_intq.h) -- the reciprocal-then-redo rule for x / scale included -- so the fp32 result is bit-identical to
//     fp8q_int_quantize_f32 on the widened input.  Ranges (delta, zero_float, the sign byte, row min / max) are fp32.
//   - y_type == FP8Q_DT_F32 stores that fp32 result; y_type == x_type rounds it ONCE to the storage type, round to nearest
//     even, overflow to infinity (what torch.Tensor.to(dtype) does).
//   - the fp32 value scale * (t - zp) exists before it is narrowed: F16::narrow1 / narrow2 (fp8q_half.h) hold it in a
//     register of its own, so the compiler cannot fold the last multiplication and the conversion into v_fma_mixlo_f16,
//     which would round the exact product once to fp16.
//   - this is deliberately NOT the reference's arithmetic on a half tensor: with a 0-dim delta ATen rounds every op to the
//     half type.  It is the contract the FP8 half lane has: widen, compute in fp32, round once.
//
// Kernel:
//   k_inth16_quant<T, YF32, RANGE, PC, NT>  k_int_quant's geometry on 2-byte elements: one 4096-element chunk per block
//                 (8 KiB of x), neighbouring blocks on neighbouring chunks, chunk_setup() of fp8q_intq.h as it is -- the
//                 sign, the channel constants of the rows overlapping the chunk in LDS, RANGE: the block in whose chunk a
//                 row starts writes that row's delta / zero_float, block 0 the sign.  A chunk starts a multiple of 8 KiB
//                 behind x, so every chunk has x's phase against the 16-byte grid: the first h (<= 7) elements up to the
//                 boundary and the last (<= 7) behind the last whole group are scalars, the rest are groups of 8 elements,
//                 one 16-byte load per lane and group, the (up to) two groups of a lane in flight together.  Every element
//                 takes the constants of its own row (Chunk::at), so rows of any length and phase -- several rows per
//                 group included -- need no second path.  The output goes out as 16 bytes (half) or 2 x 16 bytes (fp32) per
//                 group at the alignment y happens to have: y need not share x's phase, and y == x (same type) is safe
//                 because a lane writes only what it has read.
// widen8 / store_half8 are fp8q_half.h's, the fixed-range argument block is int_fixed_args() of fp8q_intq.h.
// The per-channel current_minmax entry runs fp8q_minmax_h16's row scan (fp8q_h16.hip), then the RANGE launch.
// HBM traffic per element: 4 B (half out) or 6 B (fp32 out); with the min/max scan 2 B more.
#include "fp8q_common.h"
#include "fp8q_half.h"
#include "fp8q_intq.h"

namespace {

constexpr int kGroupsPerLane = kIntChunk / 8 / kBlock;   // 2

template <class T, bool YF32, bool PC, bool NT>
__device__ __forceinline__ void chunk_walk_h16(const uint16_t *x, void *y, const Chunk &c, int h)   // (y may be x)
{
    const int tid = threadIdx.x;
    const int len = (int)(c.e1 - c.e0);
    const int ng = len > h ? (len - h) >> 3 : 0;                 // whole groups of this chunk (<= 512)
    const u4v *xv = reinterpret_cast<const u4v *>(x + c.e0 + h);
    u4v v[kGroupsPerLane];
#pragma unroll
    for (int u = 0; u < kGroupsPerLane; ++u)
        if (tid + u * kBlock < ng) v[u] = ldv<NT>(xv + tid + u * kBlock);

    // the scalars around the groups
    const int tail0 = h + 8 * ng;
    int s = -1;
    if (tid < h)
        s = tid;
    else if (tid >= 32 && tail0 + (tid - 32) < len)
        s = tail0 + (tid - 32);
    if (s >= 0 && s < len)
        store1<T, YF32>(y, c.e0 + s, int_one(T::widen1(x[c.e0 + s]), c.at<PC>(s), c.lo, c.hi));

#pragma unroll
    for (int u = 0; u < kGroupsPerLane; ++u) {
        const int g = tid + u * kBlock;
        if (g >= ng) break;
        const int off = h + 8 * g;
        float e[8];
        widen8<T>(v[u], e);
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = int_one(e[j], c.at<PC>(off + j), c.lo, c.hi);
        if (YF32) {
            float *yo = reinterpret_cast<float *>(y) + c.e0 + off;
            st16u<NT>(yo, vf4{e[0], e[1], e[2], e[3]});
            st16u<NT>(yo + 4, vf4{e[4], e[5], e[6], e[7]});
        } else {
            store_half8<T, NT>(reinterpret_cast<uint16_t *>(y) + c.e0 + off, e);
        }
    }
}

template <class T, bool YF32, bool RANGE, bool PC, bool NT>
__global__ void __launch_bounds__(kBlock)
k_inth16_quant(const uint16_t *x, void *y, IntArgs a, int h)
{
    extern __shared__ float4 kc[];    // nc_max channel constants
    auto range = [&](int64_t row, bool starts, float hi) -> Range {
        return RANGE ? SetRange{a}(row, starts, hi) : ReadRange{a}(row, starts, hi);
    };
    const Chunk c = chunk_setup<PC>(a, kc, range, RANGE && a.sign_inline);
    chunk_walk_h16<T, YF32, PC, NT>(x, y, c, h);
}

template <class T, bool YF32, bool RANGE, bool PC>
void quant_launch_nt(const uint16_t *x, void *y, const IntArgs &a, hipStream_t st)
{
    const IntPlan p = int_plan(a, false, 2);
    const dim3 g(p.grid_x), b(kBlock);
    const size_t shmem = p.lds_bytes;
    const int h = (int)(((16 - ((uintptr_t)x & 15)) & 15) >> 1);   // elements in front of x's 16-byte boundary
    if (p.nt)
        hipLaunchKernelGGL((k_inth16_quant<T, YF32, RANGE, PC, true>), g, b, shmem, st, x, y, a, h);
    else
        hipLaunchKernelGGL((k_inth16_quant<T, YF32, RANGE, PC, false>), g, b, shmem, st, x, y, a, h);
}

// the quantize launch; `range`: a.a / a.b are (x_min, x_max) and the launch also writes delta (zero_float, sign)
template <class T, bool YF32>
int quant_launch(bool range, const uint16_t *x, void *y, int64_t C, int64_t inner, IntArgs a, hipStream_t st)
{
    const bool pc = a.C > 1;
    int_geometry(a, C, inner, pc);
    if (range && pc) quant_launch_nt<T, YF32, true, true>(x, y, a, st);
    else if (range) quant_launch_nt<T, YF32, true, false>(x, y, a, st);
    else if (pc) quant_launch_nt<T, YF32, false, true>(x, y, a, st);
    else quant_launch_nt<T, YF32, false, false>(x, y, a, st);
    return launch_rc();
}

int quant_dispatch(bool range, const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const IntArgs &a,
                   hipStream_t st)
{
    const uint16_t *xs = (const uint16_t *)x;
    const bool yf32 = y_type == FP8Q_DT_F32;
    if (x_type == FP8Q_DT_F16)
        return yf32 ? quant_launch<F16, true>(range, xs, y, C, inner, a, st) : quant_launch<F16, false>(range, xs, y, C, inner, a, st);
    return yf32 ? quant_launch<BF16, true>(range, xs, y, C, inner, a, st) : quant_launch<BF16, false>(range, xs, y, C, inner, a, st);
}

// argument checks shared by the entry points (everything is reported before any launch)
int check_xy(const void *x, const void *y, int x_type, int y_type, int64_t C, int64_t inner, int64_t n_range)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    if (int rc = int_check_x(x, y, C, inner, n_range)) return rc;
    if (((uintptr_t)x & 1) || ((uintptr_t)y & (y_type == FP8Q_DT_F32 ? 3 : 1))) return FP8Q_EINVAL;
    return FP8Q_OK;
}

}  // namespace

extern "C" {

int fp8q_int_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *delta,
                          const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                          int symmetric, float eps, fp8q_stream_t stream)
{
    if (int rc = check_xy(x, y, x_type, y_type, C, inner, n_delta)) return rc;
    IntArgs a = {};
    if (int rc = int_fixed_args(a, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps)) return rc;
    return quant_dispatch(false, x, y, x_type, y_type, C, inner, a, (hipStream_t)stream);
}

int fp8q_int_range_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner,
                                const float *x_min, const float *x_max, int64_t n_range, float *delta, float *zero_float,
                                unsigned char *signed_flag, int n_bits, int symmetric, float eps, fp8q_stream_t stream)
{
    if (int rc = check_xy(x, y, x_type, y_type, C, inner, n_range)) return rc;
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
    return quant_dispatch(true, x, y, x_type, y_type, C, inner, a, st);
}

int fp8q_int_minmax_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, float *row_min,
                                 float *row_max, float *delta, float *zero_float, unsigned char *signed_flag, int n_bits,
                                 int symmetric, float eps, void *ws, size_t ws_bytes, fp8q_stream_t stream)
{
    if (int rc = check_xy(x, y, x_type, y_type, C, inner, C)) return rc;
    if (!row_min || !row_max || !delta || (symmetric ? !signed_flag : !zero_float)) return FP8Q_EINVAL;
    IntGrid probe;
    if (int rc = make_int_grid(n_bits, probe)) return rc;
    if (int rc = fp8q_minmax_h16(x, x_type, C, inner, row_min, row_max, nullptr, FP8Q_FOLD_CURRENT, 0.0, 1, ws, ws_bytes,
                                 stream))
        return rc;
    return fp8q_int_range_quantize_h16(x, y, x_type, y_type, C, inner, row_min, row_max, C, delta, zero_float, signed_flag,
                                       n_bits, symmetric, eps, stream);
}

}  // extern "C"
