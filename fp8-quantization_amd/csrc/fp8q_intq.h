// fp8q_intq.h -- what the uniform quantizers' forward (fp8q_int.hip; fp8q_inth16.hip on fp16 / bf16 tensors), backward
// (fp8q_intgrad.hip) and integer codes (fp8q_intcodec.hip; fp8q_codec_h16.hip on fp16 / bf16 tensors) share: torch's
// min / max / clamp, the integer grid of n bits, the channel constants, the integer level and the quantized value of an
// element, the code of an element and the value of a code, a row's range from (x_min, x_max), and the geometry of the
// chunked kernels (k_int_quant, k_inth16_quant, k_int_level, k_int_encode, k_int_decode): one aligned 4096-element chunk
// per block, its prologue (sign, grid ends, the channel constants in LDS, the channel of an element by magic division),
// the fp32 -> fp32 streaming loop, and the host side of their launch -- int_fixed_args(): the argument block of every
// fixed-range entry point, int_geometry() / int_sign_inline() / int_vec16() / int_plan(): the launch decisions, which the launches
// consume and fp8q_chunk_route (fp8q_int.hip) reports -- and pack_codes / code_at, the dwords of 1- and 2-byte codes.  Internal
// linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"

// k_int_sign (fp8q_int.hip): the global sign of a symmetric per-channel range, for the range-setting launches of every lane
int fp8q_int_sign_launch(const float *xmin, int64_t C, unsigned char *sflag, hipStream_t st);

namespace {

constexpr int kSignInline = 2048;     // symmetric per-channel: up to here every block reduces the xmin vector itself

__device__ __forceinline__ float t_min(float a, float b)   // torch.min(a, b) of the scalar loop: a unless b < a
{
    return (a != a) ? a : ((b != b) ? b : (b < a ? b : a));
}
__device__ __forceinline__ float t_max(float a, float b)
{
    return (a != a) ? a : ((b != b) ? b : (b > a ? b : a));
}
__device__ __forceinline__ float t_clamp(float v, float lo, float hi)   // torch.clamp: NaN passes, v when equal
{
    return (v != v) ? v : (v < lo ? lo : (v > hi ? hi : v));
}

// [int_min, int_max] of n bits: [n_lo_s, n_hi_s] when signed (a symmetric quantizer whose sign is set), [0, n_hi_u] otherwise
struct IntGrid {
    float n_hi_u;            // 2^n - 1
    float n_hi_s;            // 2^(n-1) - 1
    float n_lo_s;            // -2^(n-1)

    __device__ __forceinline__ float lo(bool sgn) const { return sgn ? n_lo_s : 0.0f; }
    __device__ __forceinline__ float hi(bool sgn) const { return sgn ? n_hi_s : n_hi_u; }
};

inline int make_int_grid(int n_bits, IntGrid &g)
{
    if (n_bits < 2 || n_bits > 16) return FP8Q_EUNSUPPORTED;
    g.n_hi_u = ldexpf(1.0f, n_bits) - 1.0f;
    g.n_hi_s = ldexpf(1.0f, n_bits - 1) - 1.0f;
    g.n_lo_s = -ldexpf(1.0f, n_bits - 1);
    return FP8Q_OK;
}

// the sign of a symmetric quantizer, as any lane reads it from the device byte
__device__ __forceinline__ bool sign_byte(int symmetric, const unsigned char *sflag)
{
    return symmetric && sflag[0] != 0;
}

// {scale, 1/scale, zp, -}
__device__ __forceinline__ float4 consts_of(float delta, float zf, bool symmetric, float lo, float hi, float eps)
{
    const float s = t_max(delta, eps);
    const float zp = symmetric ? 0.0f : t_clamp(rintf(zf), lo, hi);
    return make_float4(s, 1.0f / s, zp, 0.0f);
}

// t = clamp(rint(v / scale) + zp, lo, hi), k = consts_of(): the ONE definition of the rounding (the reciprocal-then-redo
// rule is derived at the top of fp8q_int.hip).  int_one() dequantizes it, fp8q_intcodec.hip stores it.
__device__ __forceinline__ float int_level(float v, const float4 k, float lo, float hi)
{
    const float q0 = v * k.y;
    float rq = rintf(q0);
    if (fabsf(q0 - rq) >= 0.5f - fabsf(q0) * 0x1p-20f) rq = rintf(v / k.x);
    return t_clamp(rq + k.z, lo, hi);
}

// y = scale * (t - zp): the quantize-dequantize of one element
__device__ __forceinline__ float int_one(float v, const float4 k, float lo, float hi)
{
    const float t = int_level(v, k, lo, hi);
    return k.x * (t - k.z);
}

// ---- the integer codes (fp8q_intcodec.hip; fp8q_codec_h16.hip on fp16 / bf16 tensors) ----
// the two's-complement bits of an element's level (the caller keeps the low 8 or 16)
__device__ __forceinline__ uint32_t code_of(float v, const float4 k, float lo, float hi)
{
    float t = int_level(v, k, lo, hi);
    t = (t != t) ? k.z : t;
    t = (t != t) ? 0.0f : t;
    return (uint32_t)(int)t;      // an integer in [-32768, 65535]: the conversion is exact
}

// the value of a code of W bytes, read as signed when sgn
template <int W>
__device__ __forceinline__ float value_of(uint32_t code, bool sgn, const float4 k)
{
    const int iv = sgn ? (W == 1 ? (int)(int8_t)code : (int)(int16_t)code) : (int)code;
    return k.x * ((float)iv - k.z);
}

// 4 / W codes of W bytes (each masked to its width) as a dword, the first in the low bits -- and code j of such a dword
template <int W>
__device__ __forceinline__ uint32_t pack_codes(const uint32_t *q)
{
    if constexpr (W == 1) return q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    else return q[0] | (q[1] << 16);
}
template <int W>
__device__ __forceinline__ uint32_t code_at(uint32_t w, int j)
{
    const uint32_t s = w >> (8 * W * j);
    return j == 4 / W - 1 ? s : s & (W == 1 ? 255u : 65535u);
}

// ---------------------------------------------------------------------------------------------
// The chunked kernels
// ---------------------------------------------------------------------------------------------
constexpr int kIntChunk = 4096;       // elements per block: 16 KiB of fp32

struct IntArgs {
    const float *a;          // delta [1] or [C] | range-setting launches: x_min
    const float *b;          // zero_float (asymmetric) | range-setting launches: x_max
    unsigned char *sflag;    // symmetric: the sign (read; range-setting launches with an inline fold: written by block 0)
    int64_t n;               // elements
    int inner;               // row length (PC)
    uint32_t magic;          // l / inner for l < inner + 4096 (inner < 4096)
    int nc_max;              // LDS entries per block
    int symmetric;
    float eps;
    IntGrid grid;
    // range-setting launches (fp8q_int.hip) only
    float *delta_out;        // delta written here
    float *zf_out;           // asymmetric: zero_float written here
    int64_t C;               // rows of the range vectors (1: per tensor)
    int sign_inline;         // symmetric: fold the sign from the x_min vector in every block
};

// the sign of a symmetric range: no NaN in x_min and some x_min < 0 (x_min' = min(x_min, 0) has the same predicates)
__device__ __forceinline__ bool block_sign(const float *__restrict__ xmin, int64_t C)
{
    int neg = 0, nan = 0;
    for (int64_t i = threadIdx.x; i < C; i += blockDim.x) {
        const float v = xmin[i];
        neg |= v < 0.0f;
        nan |= v != v;
    }
    neg = __syncthreads_or(neg);
    nan = __syncthreads_or(nan);
    return neg && !nan;
}

// a block's copy of the symmetric sign (false: asymmetric).  `fold`: this launch sets the range and folds the sign from
// its x_min vector (`pc`: of more than one entry) in every block, block 0 reporting it; otherwise the device byte, read
// once per block.
__device__ __forceinline__ bool int_sign(const IntArgs &a, bool fold, bool pc)
{
    __shared__ int s_sign;
    if (!a.symmetric) return false;
    if (fold) {
        const bool sgn = pc ? block_sign(a.a, a.C) : (a.a[0] < 0.0f);
        if (blockIdx.x == 0 && threadIdx.x == 0) a.sflag[0] = (unsigned char)sgn;
        return sgn;
    }
    if (threadIdx.x == 0) s_sign = sign_byte(a.symmetric, a.sflag);
    __syncthreads();
    return s_sign != 0;
}

struct Range {
    float delta, zf;
};

// a row's (delta, zero_float) as the fixed-range kernels have it: read
struct ReadRange {
    const IntArgs &a;
    __device__ __forceinline__ Range operator()(int64_t row, bool, float) const
    {
        return Range{a.a[row], a.symmetric ? 0.0f : a.b[row]};
    }
};

// set_quant_range of one row: (x_min, x_max) -> (delta, zero_float); hi: int_max of the quantizer's sign
__device__ __forceinline__ Range range_of(float xmin, float xmax, bool symmetric, float int_max, float eps)
{
    const float mn = t_min(xmin, 0.0f);
    const float mx = t_max(xmax, eps);
    Range r;
    if (symmetric) {
        r.delta = t_max(fabsf(mn), mx) / int_max;
        r.zf = 0.0f;
    } else {
        r.delta = (mx - mn) / int_max;
        r.zf = -mn / r.delta;
    }
    return r;
}

// ... and as the range-setting launches have it: from (x_min, x_max) = (a.a, a.b); the block in whose chunk the row starts
// reports it
struct SetRange {
    const IntArgs &a;
    __device__ __forceinline__ Range operator()(int64_t row, bool starts, float hi) const
    {
        const Range r = range_of(a.a[row], a.b[row], a.symmetric, hi, a.eps);
        if (starts) {
            a.delta_out[row] = r.delta;
            if (!a.symmetric) a.zf_out[row] = r.zf;
        }
        return r;
    }
};

// what a block knows about its chunk [e0, e1)
struct Chunk {
    int64_t e0, e1;
    const float4 *kc;
    float4 k0;
    float lo, hi;
    int phase, inner;
    uint32_t magic;
    bool sgn;

    // channel constants of the element at offset `off` from e0
    template <bool PC>
    __device__ __forceinline__ float4 at(int off) const
    {
        if (!PC) return k0;
        const uint32_t l = (uint32_t)(phase + off);
        const int ch = inner >= kIntChunk ? (int)(l >= (uint32_t)inner) : div_small(l, magic);
        return kc[ch];
    }
};

// The rows of a block's chunk for a lane without sign or grid (the OCP FP8 lane, fp8q_ocp.hip: {scale, 1/scale}): the
// chunk's ends, the phase of its first row, and the constants of every row overlapping it in kc (nc_max float4 of LDS), one
// lane per row: kc[i] = consts(row, starts) -- `starts`: the row begins in this chunk (per tensor: in block 0), so a launch
// that reports something per row reports it from here.
template <bool PC, typename ConstsOf>
__device__ __forceinline__ void chunk_rows(Chunk &c, const IntArgs &a, float4 *kc, ConstsOf consts)
{
    const int tid = threadIdx.x;
    c.e0 = (int64_t)blockIdx.x * kIntChunk;
    c.e1 = c.e0 + kIntChunk < a.n ? c.e0 + kIntChunk : a.n;
    const int64_t c_lo = PC ? c.e0 / a.inner : 0;
    c.phase = PC ? (int)(c.e0 - c_lo * a.inner) : 0;
    c.inner = a.inner;
    c.magic = a.magic;
    const int nc = PC ? (int)((c.e1 - 1) / a.inner - c_lo) + 1 : 1;
    for (int i = tid; i < nc; i += kBlock) {
        const int64_t row = c_lo + i;
        kc[i] = consts(row, PC ? row * a.inner >= c.e0 : blockIdx.x == 0);
    }
    __syncthreads();
    c.kc = kc;
    c.k0 = kc[0];
}

// The prologue of a block of the INT kernels.  kc: nc_max float4 of LDS.  range(row, starts, hi) yields a row's (delta,
// zero_float) -- `starts`: the row begins in this chunk, so a range-setting launch reports it from here -- and fold_sign is
// int_sign()'s.  (The geometry is chunk_rows()'s, written out: the sign's barrier sits between the chunk's ends and its rows.)
template <bool PC, typename RangeOf>
__device__ __forceinline__ Chunk chunk_setup(const IntArgs &a, float4 *kc, RangeOf range, bool fold_sign = false)
{
    const int tid = threadIdx.x;
    Chunk c;
    c.e0 = (int64_t)blockIdx.x * kIntChunk;
    c.e1 = c.e0 + kIntChunk < a.n ? c.e0 + kIntChunk : a.n;
    c.sgn = int_sign(a, fold_sign, PC);
    c.lo = a.grid.lo(c.sgn);
    c.hi = a.grid.hi(c.sgn);
    const int64_t c_lo = PC ? c.e0 / a.inner : 0;
    c.phase = PC ? (int)(c.e0 - c_lo * a.inner) : 0;
    c.inner = a.inner;
    c.magic = a.magic;
    const int nc = PC ? (int)((c.e1 - 1) / a.inner - c_lo) + 1 : 1;
    for (int i = tid; i < nc; i += kBlock) {
        const int64_t row = c_lo + i;
        const Range r = range(row, PC ? row * a.inner >= c.e0 : blockIdx.x == 0, c.hi);
        kc[i] = consts_of(r.delta, r.zf, a.symmetric, c.lo, c.hi, a.eps);
    }
    __syncthreads();
    c.kc = kc;
    c.k0 = kc[0];
    return c;
}

// y[e] = OP(x[e], the constants of e's channel, lo, hi) over the chunk.  VEC (x and y 16-byte aligned; e0 is a multiple of
// 4096, so groups of 4 are aligned): a full chunk with its four 16-byte loads in flight, a partial one group by group, the
// <= 3 elements behind the last group one by one.  !VEC: element by element.
template <bool PC, bool VEC, bool NT, float (*OP)(float, const float4, float, float)>
__device__ __forceinline__ void chunk_walk(const float *__restrict__ x, float *__restrict__ y, const Chunk &c)
{
    const int tid = threadIdx.x;
    int64_t tail = c.e0;
    if (VEC) {
        const int ngroups = (int)((c.e1 - c.e0) >> 2);
        const vf4 *xv = reinterpret_cast<const vf4 *>(x + c.e0);
        vf4 *yv = reinterpret_cast<vf4 *>(y + c.e0);
        auto op4 = [&](const vf4 v, int off) -> vf4 {
            return vf4{OP(v.x, c.at<PC>(off), c.lo, c.hi), OP(v.y, c.at<PC>(off + 1), c.lo, c.hi),
                       OP(v.z, c.at<PC>(off + 2), c.lo, c.hi), OP(v.w, c.at<PC>(off + 3), c.lo, c.hi)};
        };
        if (ngroups == kIntChunk / 4) {
            vf4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = ld16<NT>(xv + u * kBlock + tid);
#pragma unroll
            for (int u = 0; u < 4; ++u) st16<NT>(yv + u * kBlock + tid, op4(v[u], 4 * (u * kBlock + tid)));
        } else {
            for (int g = tid; g < ngroups; g += kBlock) st16<NT>(yv + g, op4(ld16<NT>(xv + g), 4 * g));
        }
        tail = c.e0 + 4 * (int64_t)ngroups;
    }
    for (int64_t e = tail + tid; e < c.e1; e += kBlock) y[e] = OP(x[e], c.at<PC>((int)(e - c.e0)), c.lo, c.hi);
}

// ---- host side ----
// argument checks shared by the chunked entry points: C rows of `inner` elements, a range of 1 or C entries
inline int int_check_x(const void *x, const void *y, int64_t C, int64_t inner, int64_t n_range)
{
    if (!x || !y || C <= 0 || inner <= 0 || (n_range != 1 && n_range != C)) return FP8Q_EINVAL;
    if ((n_range > 1 && inner > INT32_MAX) || C > INT64_MAX / inner || cdiv(C * inner, kIntChunk) > (int64_t)UINT32_MAX)
        return FP8Q_EINVAL;
    return FP8Q_OK;
}

// the argument block of a fixed-range launch: the range buffers are there, the grid of n_bits, the range as the kernels read
// it (ReadRange); the sign byte is only read
inline int int_fixed_args(IntArgs &a, const float *delta, const float *zero_float, int64_t n_delta,
                          const unsigned char *signed_flag, int n_bits, int symmetric, float eps)
{
    if (!delta || (symmetric ? !signed_flag : !zero_float)) return FP8Q_EINVAL;
    if (int rc = make_int_grid(n_bits, a.grid)) return rc;
    a.a = delta;
    a.b = zero_float;
    a.sflag = const_cast<unsigned char *>(signed_flag);
    a.C = n_delta;
    a.symmetric = symmetric != 0;
    a.eps = eps;
    return FP8Q_OK;
}

// the chunk geometry of C rows of `inner` elements; pc: one range entry per row
inline void int_geometry(IntArgs &a, int64_t C, int64_t inner, bool pc)
{
    a.n = C * inner;
    a.inner = pc ? (int)inner : 1;
    a.magic = pc ? magic_of((int)inner) : 0u;
    a.nc_max = pc ? (int)(kIntChunk / inner + 2 < C ? kIntChunk / inner + 2 : C) : 1;
}

// RANGE launches of the symmetric per-channel case: the blocks fold the sign themselves up to kSignInline entries
inline bool int_sign_inline(int symmetric, int64_t C) { return !(symmetric && C > kSignInline); }

// ... and the sign first when they cannot
inline int int_sign_prepass(IntArgs &a, hipStream_t st)
{
    a.sign_inline = int_sign_inline(a.symmetric, a.C);
    if (a.sign_inline) return FP8Q_OK;
    return fp8q_int_sign_launch(a.a, a.C, a.sflag, st);
}

// both sides of a launch on a 16-byte boundary: what the VEC instances of the fp32 kernels need
inline bool int_vec16(const void *in, const void *out) { return (((uintptr_t)in | (uintptr_t)out) & 15) == 0; }

// What a chunked launch is made with, from int_geometry()'s block: one block per chunk, nc_max float4 of dynamic LDS, the
// nontemporal instance from kNtBytes of the streamed tensor (elem_bytes per element: 4, or 2 on fp16 / bf16 tensors, whose
// kernels walk from the 16-byte boundary and have no VEC instance).  FP8Q_INT_LAUNCH and the half launchers consume it;
// fp8q_chunk_route reports it.
struct IntPlan {
    unsigned grid_x;
    size_t lds_bytes;
    bool vec, nt;
};

inline IntPlan int_plan(const IntArgs &a, bool vec, int elem_bytes)
{
    IntPlan p;
    p.grid_x = (unsigned)cdiv(a.n, kIntChunk);
    p.lds_bytes = (size_t)a.nc_max * sizeof(float4);
    p.vec = vec && elem_bytes == 4;
    p.nt = a.n * elem_bytes >= kNtBytes;
    return p;
}

// One block per chunk of K<..., VEC, NT>(in, out, a).  vec: both sides on their vector word; NT from the tensor's size.
#define FP8Q_INT_LAUNCH(vec, in, out, a, st, K, ...)                                                                   \
    do {                                                                                                              \
        const IntPlan p_ = int_plan(a, vec, 4);                                                                       \
        const dim3 g_(p_.grid_x), b_(kBlock);                                                                         \
        if (p_.vec && p_.nt) hipLaunchKernelGGL((K<__VA_ARGS__, true, true>), g_, b_, p_.lds_bytes, st, in, out, a);  \
        else if (p_.vec) hipLaunchKernelGGL((K<__VA_ARGS__, true, false>), g_, b_, p_.lds_bytes, st, in, out, a);     \
        else hipLaunchKernelGGL((K<__VA_ARGS__, false, false>), g_, b_, p_.lds_bytes, st, in, out, a);                \
    } while (0)

}  // namespace
