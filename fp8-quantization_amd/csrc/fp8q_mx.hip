// fp8q_mx.hip -- the microscaling (MX) lane (gfx950 only): blocks of 32 elements along the last dimension under ONE E8M0
// power-of-two scale byte each, elements in OCP E4M3FN, E5M2, the 6-bit E2M3 / E3M2 or the 4-bit E2M1 -- the operand forms of
// gfx950's scaled matrix instructions (v_mfma_scale_f32_*_f8f6f4) and of torch.float8_e8m0fnu / torch.float4_e2m1fn_x2 (torch
// has no 6-bit dtype).  Nothing here multiplies matrices; the lane makes, reads and fake-quantizes the operands.
//
// Arithmetic contract (include/fp8q.h states it for callers).  The tensor is [R, K], K contiguous; row r is cut into the
// blocks [32j, min(32j + 32, K)): the last block of a row may be short, no block crosses a row.
//   format   emax   fmax    mantissa field of fmax
//   E4M3FN     8     448    0x600000
//   E5M2      15   57344    0x600000
//   E2M1       2       6    0x400000
//   E2M3       2     7.5    0x700000        s1 e2 m3, bias 1
//   E3M2       4      28    0x600000        s1 e3 m2, bias 3
//   (the ids: E4M3FN 0, E5M2 1, E2M1 2, E2M3 4, E3M2 5; id 3 stays unassigned and FP8Q_EUNSUPPORTED like every other number)
//   m    = the largest bits(|x|) of the block, compared as unsigned integers (so NaN and inf patterns are the largest)
//   E    = m >> 23, man = m & 0x7fffff
//   code = max(E - emax + bump, 0)           bump = 0 (floor, the OCP MX v1.0 rule X = 2^(floor(log2 amax) - emax)) or
//                                            man > man_fmax (ceil: the smallest power of two under which nothing saturates)
//          0xFF when E == 255 (a NaN or an infinity anywhere in the block); a zero or subnormal-only block gives 0
//   X    = 2^(code - 127) as fp32            code 0 is the subnormal 0x00400000, 0xFF is NaN
//   q    = clamp(x * 2^(127 - code), -fmax, fmax)   ONE fp32 multiplication by an exactly representable power of two: exact
//                                            unless it lands in fp32's subnormal range, far below every format's smallest
//                                            midpoint, where the element is a zero of x's sign either way
//   elem = RNE(q) in the element format      subnormals included, -0 keeps its sign (0x80 / 0x8); a 0xFF block stores 0x7F
//                                            (FP8) / 0x0 (FP6, FP4) everywhere
//   E2M1: the codes 0..7 are {0, .5, 1, 1.5, 2, 3, 4, 6}, the sign in bit 3, a tie goes to the even code; two elements
//   share a byte, the even-indexed one in the low nibble (K must be even)
//   FP6: the magnitude code c is the low 5 bits, the sign bit 5, no NaN and no infinity among the 64 codes, a tie goes to the
//   even code, -0 is 0x20.  E2M3: e = c >> 3, m = c & 7, value m * 0.125 (e == 0) or (1 + m / 8) * 2^(e - 1); E3M2: e = c >> 2,
//   m = c & 3, value m * 0.0625 (e == 0) or (1 + m / 4) * 2^(e - 3).  The codes of a row are one little-endian bit string,
//   element i in bits [6i, 6i + 6): four elements are three bytes, b0 = e0 | e1 << 6, b1 = e1 >> 2 | e2 << 4,
//   b2 = e2 >> 4 | e3 << 2 (K % 4 == 0 is required: no byte is shared between rows, every block starts on a byte); a full
//   block is 24 bytes, the 6-VGPR operand of the matrix instruction; codes are [R, 3K / 4] bytes
//   decode(elem) = value(elem) * X           ONE fp32 multiplication, subnormal products kept; every element of a 0xFF block
//                                            is NaN; a half output rounds that product once
//   quantize(x)  = decode(encode(x))         the same device functions in one pass
//
// What does the conversions.  FP8: v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 on the clamped q and v_cvt_f32_fp8 / v_cvt_f32_bf8,
// exactly as fp8q_ocp.hip uses them (RNE, subnormals, -0, E5M2's infinities on decode).  FP4: integer arithmetic -- seven
// comparisons against the midpoints {.25, .75, 1.25, 1.75, 2.5, 3.5, 5}, `>=` at those whose upper neighbour is the even
// code -- and the value's bits built from the code.  FP6: one integer routine for both formats, parameterised by the mantissa
// width M (fp6_code / fp6_value): a normal q is rebiased and rounded on its bits, the carry running into the exponent; a
// subnormal one is rounded by one fp32 addition of 2^(24 - bias - M), whose unit in the last place is the grid's step; the
// value is the code's bits read as an fp32 (subnormal where e == 0) times 2^(127 - bias), which is exact.  gfx950's scaled
// conversions (v_cvt_scalef32_pk_fp4_f32, v_cvt_scalef32_pk32_fp6_f32 and kin) are NOT used: nothing has shown yet that they
// reproduce this contract on subnormal inputs and ties.
//
// Kernels.  k_mx<MODE, F, IN, OUT, NT>, the fast route: K % 32 == 0 and x / y / codes 16-byte aligned.  Then blocks tile the
// flat tensor, block b covers elements [32b, 32b + 32) and owns scale byte b, and a workgroup takes 4096 consecutive elements.
//   encode: a lane owns 16 consecutive elements, its 16-byte loads (four of fp32, two of half) issued before any arithmetic;
//           the two lanes of a block exchange their integer maxima in one DPP step; 16 FP8 codes leave as ONE
//           16-byte word, 16 FP4 codes as one 8-byte word, 16 FP6 codes as three dwords at byte 12 * lane of the chunk's
//           codes (4-byte aligned; a wave writes 768 contiguous bytes); the even lane stores the block's scale byte (a plain
//           1-byte store)
//   decode, quantize: lane <-> group of 4 elements, four groups per lane 1024 elements apart, so that every store instruction
//           of a wave writes whole lines; quantize folds the maxima of a block's 8 lanes in three DPP steps; decode reads the
//           block's scale byte in each of its 8 lanes (one byte, broadcast by the cache)
//           FP6 decode keeps that geometry: a group's three code bytes lie at byte 3g, so a lane fetches them from the one
//           or two aligned dwords that hold them (v_alignbyte_b32; the second dword only where the group crosses into it) and
//           the value stores stay as they are.  The other candidate -- the encode geometry, a lane of 16 elements with three
//           aligned dword loads and its own 16-byte value stores -- measured 1.6x (bfloat16) to 4.8x (float32) slower on
//           [8192, 8192] (profiles/mx6_mb.txt): each of a wave's store instructions then touches 64 lines a quarter each
// Every element is read exactly once.  NT: nontemporal loads and stores from 64 MiB (kNtBytes), the rule of the INT kernels.
// k_mx_plain<MODE, F, IN, OUT>, the general route (ragged K, misaligned views): one lane per block, element by element (FP4:
// two elements and a byte, FP6: four elements and three bytes at a time, the code side at any address), the block read twice by
// encode and quantize.  A correctness path; no rate is claimed for it.
// One launch per call, nothing read back, no allocation, no workspace.
// HBM traffic per element, fast route: FP8 encode 4 + 1 + 1/32 B (2 + 1 + 1/32 from half), FP6 encode 4 + 3/4 + 1/32, FP4
// encode 4 + 1/2 + 1/32.
// Shared with fp8q_ocp.hip through fp8q_io.h: the launch modes, the Io* element policies, Fp8Fmt (the conversion instructions)
// and io_dispatch(), the (mode, in_type, out_type) ladder that mx_launch ends in.  Shared with fp8q_mx_t.hip (the same operands
// with the blocks along dim 0) through fp8q_mxq.h: the block size, MxFmt, the scale byte and every element conversion.
#include "fp8q_common.h"
#include "fp8q_io.h"
#include "fp8q_mxq.h"

namespace {

constexpr int kMxChunk = 4096;        // elements per workgroup: 16 per lane (encode), 4 x 4 per lane (decode, quantize)

// The three code bytes of the FP6 group g (elements 4g .. 4g + 3: byte 3g of `codes`, which is 16-byte aligned) out of the one
// or two aligned dwords that hold them; the second dword is fetched only where the group crosses into it, so it holds codes too
template <bool NT>
__device__ __forceinline__ uint32_t fp6_load3(const uint8_t *codes, int64_t g)
{
    const int64_t at = 3 * g;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(codes) + (at >> 2);
    const uint32_t r = (uint32_t)at & 3u;
    const uint32_t lo = ldv<NT>(p);
    const uint32_t hi = r >= 2u ? ldv<NT>(p + 1) : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, r) & 0xffffffu;
}

struct MxArgs {
    const uint8_t *scales_in;     // decode
    uint8_t *scales_out;          // encode
    int64_t n;                    // elements
    int64_t K;                    // row length
    int64_t nb;                   // blocks per row
    int64_t blocks;               // R * nb
    int ceil_rule;
    MxSr sr;                      // the SR kernels' seed and offset
};

// ---- the fast route: n % 32 == 0, blocks tile the flat tensor, every vector word aligned ----
// SR: elem = RNE(SR(q, r)), the draws by the element's flat index (fp8q_mxq.h); an encoding lane's 16 elements are two whole
// Philox calls, a quantizing lane's group of 4 is half of one
template <int MODE, int F, class IN, class OUT, bool NT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_mx(const void *__restrict__ in, void *__restrict__ out, MxArgs a)
{
    typedef typename IN::elem in_t;
    typedef typename OUT::elem out_t;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kMxChunk;
    const int left = (int)(a.n - e0 < kMxChunk ? a.n - e0 : kMxChunk);      // a multiple of 32
    const in_t *x = static_cast<const in_t *>(in);
    out_t *y = static_cast<out_t *>(out);
    if constexpr (MODE == kEncode) {
        // lanes 2i and 2i + 1 hold block i of the chunk; `left` is a multiple of 32, so both are live or neither is, and the
        // shuffle runs in every lane
        const bool live = 16 * tid < left;
        const int64_t e = e0 + 16 * tid;
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = 0.0f;
        if (live) IN::template load16<NT>(x + e, v);
        uint32_t m = umax4(v);
#pragma unroll
        for (int g = 1; g < 4; ++g) {
            const uint32_t t = umax4(v + 4 * g);
            m = t > m ? t : m;
        }
        m = umax_xor<1>(m);
        const uint32_t sc = scale_code<F>(m, a.ceil_rule);
        uint32_t w[4];
        if constexpr (SR) {
            const uint64_t i0 = a.sr.offset + (uint64_t)e;      // a multiple of 8
            uint32_t d[8];
            mx_draw8(a.sr, i0, d);
            mx_draw8(a.sr, i0 + 8u, d + 4);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint32_t r[4];
                mx_split4(d + 2 * g, r);
                w[g] = mx_code4_sr<F>(v + 4 * g, sc, r);
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) w[g] = mx_code4<F>(v + 4 * g, sc);
        }
        if (live) {
            if constexpr (F == FP8Q_MX_E2M1) {
                stv<NT>(reinterpret_cast<u2v *>(y + (e >> 1)), u2v{w[0] | (w[1] << 16), w[2] | (w[3] << 16)});
            } else if constexpr (kFp6<F>) {
                // 96 bits at byte 12 * lane of the chunk's codes: 4-byte aligned, dword by dword
                uint32_t *c = reinterpret_cast<uint32_t *>(y + 3 * (e >> 2));
                stv<NT>(c, w[0] | (w[1] << 24));
                stv<NT>(c + 1, (w[1] >> 8) | (w[2] << 16));
                stv<NT>(c + 2, (w[2] >> 16) | (w[3] << 8));
            } else {
                stv<NT>(reinterpret_cast<u4v *>(y + e), u4v{w[0], w[1], w[2], w[3]});
            }
            if (!(tid & 1)) a.scales_out[e >> 5] = (uint8_t)sc;
        }
    } else {
        // lanes 8i .. 8i + 7 hold a block; a partial chunk ends on a block, so the folds see live lanes only -- and the loop
        // is uniform, so every lane runs them
        auto group = [&](const float *v, uint32_t w, int off, bool live) {
            uint32_t sc = 0u;
            if constexpr (MODE == kQuant) {
                uint32_t m = umax4(v);
                m = umax_xor<1>(m);
                m = umax_xor<2>(m);
                m = umax_xor<4>(m);
                sc = scale_code<F>(m, a.ceil_rule);
                if constexpr (SR) {
                    uint32_t d[2], r[4];
                    mx_draw4(a.sr, a.sr.offset + (uint64_t)(e0 + off), d);
                    mx_split4(d, r);
                    w = mx_code4_sr<F>(v, sc, r);
                } else {
                    w = mx_code4<F>(v, sc);
                }
            } else if (live) {
                sc = a.scales_in[(e0 + off) >> 5];
            }
            float r[4];
            mx_value4<F>(w, sc, r);
            if (live) OUT::template store4<NT>(y + e0 + off, r);
        };
        auto fetch = [&](float *v, uint32_t &w, int off, bool live) {
            v[0] = v[1] = v[2] = v[3] = 0.0f;
            w = 0u;
            if (!live) return;
            if constexpr (MODE == kQuant) IN::template load4<NT>(x + e0 + off, v);
            else if constexpr (F == FP8Q_MX_E2M1) w = ldv<NT>(reinterpret_cast<const uint16_t *>(x + ((e0 + off) >> 1)));
            else if constexpr (kFp6<F>) w = fp6_load3<NT>(x, (e0 + off) >> 2);
            else w = IoCodes::load4<NT>(x + e0 + off);
        };
        if (left == kMxChunk) {
            float v[4][4];
            uint32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) fetch(v[u], w[u], 4 * (u * kBlock + tid), true);
#pragma unroll
            for (int u = 0; u < 4; ++u) group(v[u], w[u], 4 * (u * kBlock + tid), true);
        } else {
            for (int base = 0; base < left; base += 4 * kBlock) {
                const int off = base + 4 * tid;
                const bool live = off < left;
                float v[4];
                uint32_t w;
                fetch(v, w, off, live);
                group(v, w, off, live);
            }
        }
    }
}

// ---- the general route: one lane per block, element by element ----
template <int MODE, int F, class IN, class OUT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_mx_plain(const void *__restrict__ in, void *__restrict__ out, MxArgs a)
{
    typedef typename IN::elem in_t;
    typedef typename OUT::elem out_t;
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= a.blocks) return;
    const int64_t row = b / a.nb, j = b - row * a.nb;
    const int64_t base = row * a.K + kMxBlock * j;
    const int len = (int)(a.K - kMxBlock * j < kMxBlock ? a.K - kMxBlock * j : kMxBlock);
    const in_t *x = static_cast<const in_t *>(in);
    out_t *y = static_cast<out_t *>(out);
    uint32_t sc;
    if constexpr (MODE == kDecode) {
        sc = a.scales_in[b];
    } else {
        uint32_t m = 0u;
        for (int i = 0; i < len; ++i) {
            const uint32_t t = abs_bits(IN::load1(x + base + i));
            m = t > m ? t : m;
        }
        sc = scale_code<F>(m, a.ceil_rule);
        if constexpr (MODE == kEncode) a.scales_out[b] = (uint8_t)sc;
    }
    // kStep elements are kBytes whole bytes of codes.  E2M1: K is even, FP6: K is a multiple of 4, so base and len are: the
    // elements of a step lie in one block, and no step shares a byte with another
    constexpr int kStep = F == FP8Q_MX_E2M1 ? 2 : (kFp6<F> ? 4 : 1);
    constexpr int kBytes = kFp6<F> ? 3 : 1;
    for (int i = 0; i < len; i += kStep) {
        const int64_t e = base + i;
        const int64_t cb = e / kStep * kBytes;
        uint32_t w = 0u;
        if constexpr (MODE == kDecode) {
#pragma unroll
            for (int k = 0; k < kBytes; ++k) w |= (uint32_t)x[cb + k] << (8 * k);
        } else {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < kStep; ++k) v[k] = IN::load1(x + e + k);
            if constexpr (SR) {
                uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < kStep; ++k) r[k] = mx_draw1(a.sr, a.sr.offset + (uint64_t)(e + k));
                w = mx_code4_sr<F>(v, sc, r) & ((1u << (8 * kBytes)) - 1u);
            } else {
                w = mx_code4<F>(v, sc) & ((1u << (8 * kBytes)) - 1u);
            }
        }
        if constexpr (MODE == kEncode) {
#pragma unroll
            for (int k = 0; k < kBytes; ++k) y[cb + k] = (uint8_t)(w >> (8 * k));
        } else {
            float r[4];
            mx_value4<F>(w, sc, r);
#pragma unroll
            for (int k = 0; k < kStep; ++k) OUT::store1(y + e + k, r[k]);
        }
    }
}

template <int MODE, int F, class IN, class OUT, bool SR>
void launch_io(const void *in, void *out, const MxArgs &a, bool fast, hipStream_t st)
{
    const dim3 b(kBlock);
    if (!fast) {
        hipLaunchKernelGGL((k_mx_plain<MODE, F, IN, OUT, SR>), dim3((unsigned)cdiv(a.blocks, kBlock)), b, 0, st, in, out, a);
        return;
    }
    const dim3 g((unsigned)cdiv(a.n, kMxChunk));
    if (a.n * 4 >= kNtBytes) hipLaunchKernelGGL((k_mx<MODE, F, IN, OUT, true, SR>), g, b, 0, st, in, out, a);
    else hipLaunchKernelGGL((k_mx<MODE, F, IN, OUT, false, SR>), g, b, 0, st, in, out, a);
}

// Argument checks (everything is reported before the launch) and the one launch.  in_type / out_type: FP8Q_DT_* of the value
// side(s), -1 for the side that holds codes.  scales: written by encode, read by decode, unused (null) by quantize.  sr: the
// seed and offset of a stochastic-rounding entry (encode, quantize), null for round to nearest even.
int mx_launch(int mode, const void *in, void *out, const uint8_t *scales, int in_type, int out_type, int64_t R, int64_t K,
              int fmt, int rounding, hipStream_t st, const MxSr *sr = nullptr)
{
    if (!in || !out || (mode != kQuant && !scales) || R <= 0 || K <= 0) return FP8Q_EINVAL;
    const bool fp6 = fmt == FP8Q_MX_E2M3 || fmt == FP8Q_MX_E3M2;
    if (fmt != FP8Q_MX_E4M3FN && fmt != FP8Q_MX_E5M2 && fmt != FP8Q_MX_E2M1 && !fp6) return FP8Q_EUNSUPPORTED;
    if (rounding != FP8Q_MX_FLOOR && rounding != FP8Q_MX_CEIL) return FP8Q_EINVAL;
    if (sr && (sr->offset & 7u)) return FP8Q_EINVAL;
    if ((fmt == FP8Q_MX_E2M1 && (K & 1)) || (fp6 && (K & 3))) return FP8Q_EINVAL;
    if (value_side_misaligned(in, in_type) || value_side_misaligned(out, out_type)) return FP8Q_EINVAL;
    const int64_t nb = cdiv(K, kMxBlock);
    if (R > INT64_MAX / K || R > INT64_MAX / nb || cdiv(R * nb, kBlock) > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    MxArgs a = {};
    a.scales_in = scales;
    a.scales_out = const_cast<uint8_t *>(scales);
    a.n = R * K;
    a.K = K;
    a.nb = nb;
    a.blocks = R * nb;
    a.ceil_rule = rounding == FP8Q_MX_CEIL;
    if (sr) a.sr = *sr;
    const bool fast = K % kMxBlock == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    io_dispatch(mode, in_type, out_type, [&](auto m, auto ti, auto to) {
        constexpr int MODE = decltype(m)::value;
        typedef decltype(ti) IN;
        typedef decltype(to) OUT;
        auto go = [&](auto sr_on) {
            constexpr bool SR = decltype(sr_on)::value;
            if (fmt == FP8Q_MX_E4M3FN) launch_io<MODE, FP8Q_MX_E4M3FN, IN, OUT, SR>(in, out, a, fast, st);
            else if (fmt == FP8Q_MX_E5M2) launch_io<MODE, FP8Q_MX_E5M2, IN, OUT, SR>(in, out, a, fast, st);
            else if (fmt == FP8Q_MX_E2M3) launch_io<MODE, FP8Q_MX_E2M3, IN, OUT, SR>(in, out, a, fast, st);
            else if (fmt == FP8Q_MX_E3M2) launch_io<MODE, FP8Q_MX_E3M2, IN, OUT, SR>(in, out, a, fast, st);
            else launch_io<MODE, FP8Q_MX_E2M1, IN, OUT, SR>(in, out, a, fast, st);
        };
        if constexpr (MODE != kDecode) {
            if (sr) {
                go(std::true_type{});
                return;
            }
        }
        go(std::false_type{});
    });
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_mx_encode_f32(const float *x, uint8_t *codes, uint8_t *scales, int64_t R, int64_t K, int fmt, int rounding,
                       fp8q_stream_t stream)
{
    return mx_launch(kEncode, x, codes, scales, FP8Q_DT_F32, -1, R, K, fmt, rounding, (hipStream_t)stream);
}

int fp8q_mx_encode_h16(const void *x, uint8_t *codes, uint8_t *scales, int x_type, int64_t R, int64_t K, int fmt,
                       int rounding, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    return mx_launch(kEncode, x, codes, scales, x_type, -1, R, K, fmt, rounding, (hipStream_t)stream);
}

int fp8q_mx_decode_f32(const uint8_t *codes, const uint8_t *scales, float *y, int64_t R, int64_t K, int fmt,
                       fp8q_stream_t stream)
{
    return mx_launch(kDecode, codes, y, scales, -1, FP8Q_DT_F32, R, K, fmt, FP8Q_MX_FLOOR, (hipStream_t)stream);
}

int fp8q_mx_decode_h16(const uint8_t *codes, const uint8_t *scales, void *y, int y_type, int64_t R, int64_t K, int fmt,
                       fp8q_stream_t stream)
{
    if (!half_type(y_type)) return FP8Q_EINVAL;
    return mx_launch(kDecode, codes, y, scales, -1, y_type, R, K, fmt, FP8Q_MX_FLOOR, (hipStream_t)stream);
}

int fp8q_mx_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, fp8q_stream_t stream)
{
    return mx_launch(kQuant, x, y, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, fmt, rounding, (hipStream_t)stream);
}

int fp8q_mx_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                         fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    return mx_launch(kQuant, x, y, nullptr, x_type, y_type, R, K, fmt, rounding, (hipStream_t)stream);
}

// ---- stochastic rounding of the elements: the twins of the four entries above that convert ----
int fp8q_mxsr_encode_f32(const float *x, uint8_t *codes, uint8_t *scales, int64_t R, int64_t K, int fmt, int rounding,
                         uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return mx_launch(kEncode, x, codes, scales, FP8Q_DT_F32, -1, R, K, fmt, rounding, (hipStream_t)stream, &sr);
}

int fp8q_mxsr_encode_h16(const void *x, uint8_t *codes, uint8_t *scales, int x_type, int64_t R, int64_t K, int fmt,
                         int rounding, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    const MxSr sr = mx_sr_args(seed, offset);
    return mx_launch(kEncode, x, codes, scales, x_type, -1, R, K, fmt, rounding, (hipStream_t)stream, &sr);
}

int fp8q_mxsr_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, uint64_t seed,
                           uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return mx_launch(kQuant, x, y, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, fmt, rounding, (hipStream_t)stream, &sr);
}

int fp8q_mxsr_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                           uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    const MxSr sr = mx_sr_args(seed, offset);
    return mx_launch(kQuant, x, y, nullptr, x_type, y_type, R, K, fmt, rounding, (hipStream_t)stream, &sr);
}

}  // extern "C"
