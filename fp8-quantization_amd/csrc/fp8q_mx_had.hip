// fp8q_mx_had.hip -- the MX lane with a block Hadamard rotation in front of the quantization (gfx950 only), blocks along the
// last dimension.  One outlier in a block of 32 sets the E8M0 scale of all 32 elements; at FP4 / FP6 the other 31 then land on
// the lowest few codes.  A random sign vector followed by the orthonormal 32 x 32 Walsh-Hadamard transform spreads the outlier
// over the block, and both operands of a product take the same rotation along the reduction dimension, so the product is
// unchanged.  include/fp8q.h states the arithmetic (fp8q_hadq.h implements it, and says why it is butterflies and not the
// matrix cores); everything after the rotation is the MX contract of fp8q_mx.hip, on the device functions of fp8q_mxq.h:
//   rotate      y = H32(x, sign_mask), or its inverse; any of fp32 / half in, any of them out
//   encode      mx_encode of the rotated block, codes and scales
//   quantize    the inverse rotation of mx_quantize of the rotated block: the result is in x's own domain
// K % 32 == 0 is required, so blocks tile the flat tensor and are never short.
//
// k_mxh<MODE, F, IN, OUT, NT, SR>, the fast route (x and y / codes 16-byte aligned): k_mx's geometries, a workgroup on 4096
// consecutive elements, because they are what makes every load and store instruction of a wave cover whole lines.
//   encode: a lane owns 16 consecutive elements, its 16-byte loads issued before any arithmetic; the lane's 16 bits of the mask,
//           stages 0 .. 3 in registers, stage 4 one DPP exchange with the partner lane, the multiplication; then k_mx's steps:
//           the integer maxima, scale_code, mx_code4 / mx_code4_sr and the packed stores
//   quantize, rotate: lane <-> group of 4, eight lanes to a block, four groups per lane 1024 elements apart; stages 0 and 1 in
//           registers, stages 2, 3 and 4 across lanes by xor 1, 2 and 4 (DPP); quantize then runs range, code and value as
//           k_mx does and the inverse the same way back.  The plain rotation takes this geometry and not the encoder's: its
//           value stores are then whole lines, which is what fp8q_mx.hip's header measured for decode
//   The mask bits of a lane depend on tid alone (a group's place in its block is tid & 7, a half block's tid & 1).
// k_mxh_plain<MODE, F, IN, OUT, SR>, the general route (misaligned views): one lane per block, its 32 values in registers, all
// five stages in the lane, code bytes one by one.  A correctness path, as k_mx_plain is.
// NT: nontemporal loads and stores from 64 MiB, the lane's rule.  One launch per call, no LDS, no workspace, every element read
// once.  The draws of stochastic rounding go by the element's flat index, which the rotation does not move.
#include "fp8q_common.h"
#include "fp8q_hadq.h"
#include "fp8q_io.h"
#include "fp8q_mxq.h"

namespace {

constexpr int kRotate = 3;            // the launch mode next to kEncode and kQuant: the rotation alone
constexpr int kMxChunk = 4096;        // elements per workgroup, as in fp8q_mx.hip

struct MxhArgs {
    uint8_t *scales_out;          // encode
    int64_t n;                    // elements, a multiple of 32
    int64_t blocks;               // n / 32
    uint32_t mask;                // the sign vector
    int inverse;                  // rotate: the inverse
    int ceil_rule;
    MxSr sr;
};

// the rotation of a group of 4 whose block lies in the 8 lanes tid & ~7 .. tid | 7: signs `pre` before, signs `post` after
__device__ __forceinline__ void had_group4(float *v, uint32_t pre, uint32_t post, int tid)
{
    had_signs<4>(v, pre);
    had_regs<4>(v);
    had_cross<1, 4>(v, (uint32_t)(tid & 1) << 31);
    had_cross<2, 4>(v, (uint32_t)(tid & 2) << 30);
    had_cross<4, 4>(v, (uint32_t)(tid & 4) << 29);
    had_norm<4>(v);
    had_signs<4>(v, post);
}

template <int MODE, int F, class IN, class OUT, bool NT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_mxh(const void *__restrict__ in, void *__restrict__ out, MxhArgs a)
{
    typedef typename IN::elem in_t;
    typedef typename OUT::elem out_t;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kMxChunk;
    const int left = (int)(a.n - e0 < kMxChunk ? a.n - e0 : kMxChunk);      // a multiple of 32
    const in_t *x = static_cast<const in_t *>(in);
    out_t *y = static_cast<out_t *>(out);
    if constexpr (MODE == kEncode) {
        // lanes 2i and 2i + 1 hold block i of the chunk: both are live or neither is, and the exchanges run in every lane
        const bool live = 16 * tid < left;
        const int64_t e = e0 + 16 * tid;
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = 0.0f;
        if (live) IN::template load16<NT>(x + e, v);
        had_signs<16>(v, a.mask >> (16 * (tid & 1)));
        had_regs<16>(v);
        had_cross<1, 16>(v, (uint32_t)(tid & 1) << 31);
        had_norm<16>(v);
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
        // lanes 8i .. 8i + 7 hold a block; a partial chunk ends on a block and the loop is uniform, so every exchange sees live
        // lanes only and runs in every lane
        const uint32_t sb = (a.mask >> (4 * (tid & 7))) & 0xfu;
        const uint32_t pre = (MODE == kQuant || !a.inverse) ? sb : 0u, post = (MODE == kRotate && a.inverse) ? sb : 0u;
        auto group = [&](float *v, int off, bool live) {
            had_group4(v, pre, post, tid);
            if constexpr (MODE == kQuant) {
                uint32_t m = umax4(v);
                m = umax_xor<1>(m);
                m = umax_xor<2>(m);
                m = umax_xor<4>(m);
                const uint32_t sc = scale_code<F>(m, a.ceil_rule);
                uint32_t w;
                if constexpr (SR) {
                    uint32_t d[2], r[4];
                    mx_draw4(a.sr, a.sr.offset + (uint64_t)(e0 + off), d);
                    mx_split4(d, r);
                    w = mx_code4_sr<F>(v, sc, r);
                } else {
                    w = mx_code4<F>(v, sc);
                }
                mx_value4<F>(w, sc, v);
                had_group4(v, 0u, sb, tid);
            }
            if (live) OUT::template store4<NT>(y + e0 + off, v);
        };
        if (left == kMxChunk) {
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) IN::template load4<NT>(x + e0 + 4 * (u * kBlock + tid), v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) group(v[u], 4 * (u * kBlock + tid), true);
        } else {
            for (int base = 0; base < left; base += 4 * kBlock) {
                const int off = base + 4 * tid;
                const bool live = off < left;
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (live) IN::template load4<NT>(x + e0 + off, v);
                group(v, off, live);
            }
        }
    }
}

// ---- the general route: one lane per block, the block in registers ----
template <int MODE, int F, class IN, class OUT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_mxh_plain(const void *__restrict__ in, void *__restrict__ out, MxhArgs a)
{
    typedef typename IN::elem in_t;
    typedef typename OUT::elem out_t;
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= a.blocks) return;
    const int64_t base = kMxBlock * b;
    const in_t *x = static_cast<const in_t *>(in);
    out_t *y = static_cast<out_t *>(out);
    float v[kMxBlock];
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i) v[i] = IN::load1(x + base + i);
    if constexpr (MODE == kRotate) {
        had_block32(v, a.inverse ? 0u : a.mask, a.inverse ? a.mask : 0u);
    } else {
        had_block32(v, a.mask, 0u);
        uint32_t m = 0u;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const uint32_t t = umax4(v + 4 * g);
            m = t > m ? t : m;
        }
        const uint32_t sc = scale_code<F>(m, a.ceil_rule);
        constexpr int kBytes = F == FP8Q_MX_E2M1 ? 2 : (kFp6<F> ? 3 : 4);       // code bytes of a group of 4
        if constexpr (MODE == kEncode) a.scales_out[b] = (uint8_t)sc;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            uint32_t w;
            if constexpr (SR) {
                uint32_t d[2], r[4];
                mx_draw4(a.sr, a.sr.offset + (uint64_t)(base + 4 * g), d);
                mx_split4(d, r);
                w = mx_code4_sr<F>(v + 4 * g, sc, r);
            } else {
                w = mx_code4<F>(v + 4 * g, sc);
            }
            if constexpr (MODE == kEncode) {
                uint8_t *cb = reinterpret_cast<uint8_t *>(y) + (8 * b + g) * kBytes;
#pragma unroll
                for (int k = 0; k < kBytes; ++k) cb[k] = (uint8_t)(w >> (8 * k));
            } else {
                mx_value4<F>(w, sc, v + 4 * g);
            }
        }
        if constexpr (MODE == kQuant) had_block32(v, 0u, a.mask);
    }
    if constexpr (MODE != kEncode) {
#pragma unroll
        for (int i = 0; i < kMxBlock; ++i) OUT::store1(y + base + i, v[i]);
    }
}

template <int MODE, int F, class IN, class OUT, bool SR>
void launch_io(const void *in, void *out, const MxhArgs &a, bool fast, hipStream_t st)
{
    const dim3 b(kBlock);
    if (!fast) {
        hipLaunchKernelGGL((k_mxh_plain<MODE, F, IN, OUT, SR>), dim3((unsigned)cdiv(a.blocks, kBlock)), b, 0, st, in, out, a);
        return;
    }
    const dim3 g((unsigned)cdiv(a.n, kMxChunk));
    if (a.n * 4 >= kNtBytes) hipLaunchKernelGGL((k_mxh<MODE, F, IN, OUT, true, SR>), g, b, 0, st, in, out, a);
    else hipLaunchKernelGGL((k_mxh<MODE, F, IN, OUT, false, SR>), g, b, 0, st, in, out, a);
}

// Argument checks (everything is reported before the launch, in mx_launch's order and with its codes) and the one launch.
// in_type / out_type: FP8Q_DT_* of the value side(s), -1 for the side that holds codes.  sr: the seed and offset of a call that
// rounds stochastically, null for round to nearest even.
int mxh_launch(int mode, const void *in, void *out, uint8_t *scales, int in_type, int out_type, int64_t R, int64_t K, int fmt,
               int rounding, uint32_t mask, int inverse, hipStream_t st, const MxSr *sr)
{
    if (!in || !out || (mode == kEncode && !scales) || R <= 0 || K <= 0) return FP8Q_EINVAL;
    if (mode != kRotate) {
        const bool fp6 = fmt == FP8Q_MX_E2M3 || fmt == FP8Q_MX_E3M2;
        if (fmt != FP8Q_MX_E4M3FN && fmt != FP8Q_MX_E5M2 && fmt != FP8Q_MX_E2M1 && !fp6) return FP8Q_EUNSUPPORTED;
        if (rounding != FP8Q_MX_FLOOR && rounding != FP8Q_MX_CEIL) return FP8Q_EINVAL;
    }
    if (sr && (sr->offset & 7u)) return FP8Q_EINVAL;
    if (K % kMxBlock) return FP8Q_EINVAL;                   // blocks are never short under a rotation
    if (value_side_misaligned(in, in_type) || value_side_misaligned(out, out_type)) return FP8Q_EINVAL;
    if (R > INT64_MAX / K || cdiv(R * (K / kMxBlock), kBlock) > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    MxhArgs a = {};
    a.scales_out = scales;
    a.n = R * K;
    a.blocks = a.n / kMxBlock;
    a.mask = mask;
    a.inverse = inverse != 0;
    a.ceil_rule = rounding == FP8Q_MX_CEIL;
    if (sr) a.sr = *sr;
    const bool fast = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    if (mode == kRotate) {
        value_io(in_type, [&](auto ti) {
            value_io(out_type, [&](auto to) {
                launch_io<kRotate, FP8Q_MX_E4M3FN, decltype(ti), decltype(to), false>(in, out, a, fast, st);
            });
        });
        return launch_rc();
    }
    io_dispatch(mode, in_type, out_type, [&](auto m, auto ti, auto to) {
        constexpr int MODE = decltype(m)::value;
        typedef decltype(ti) IN;
        typedef decltype(to) OUT;
        if constexpr (MODE != kDecode) {
            dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M3, FP8Q_MX_E3M2, FP8Q_MX_E2M1>(fmt, [&](auto fc) {
                constexpr int F = decltype(fc)::value;
                if (sr) launch_io<MODE, F, IN, OUT, true>(in, out, a, fast, st);
                else launch_io<MODE, F, IN, OUT, false>(in, out, a, fast, st);
            });
        }
    });
    return launch_rc();
}

inline bool value_type(int t) { return t == FP8Q_DT_F32 || half_type(t); }

}  // namespace

extern "C" {

int fp8q_mxh_transform_f32(const float *x, float *y, int64_t R, int64_t K, uint32_t sign_mask, int inverse,
                           fp8q_stream_t stream)
{
    return mxh_launch(kRotate, x, y, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, 0, FP8Q_MX_FLOOR, sign_mask, inverse,
                      (hipStream_t)stream, nullptr);
}

int fp8q_mxh_transform_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, uint32_t sign_mask,
                           int inverse, fp8q_stream_t stream)
{
    if (!value_type(x_type) || !value_type(y_type) || (!half_type(x_type) && !half_type(y_type))) return FP8Q_EINVAL;
    return mxh_launch(kRotate, x, y, nullptr, x_type, y_type, R, K, 0, FP8Q_MX_FLOOR, sign_mask, inverse, (hipStream_t)stream,
                      nullptr);
}

int fp8q_mxh_encode_f32(const float *x, uint8_t *codes, uint8_t *scales, int64_t R, int64_t K, int fmt, int rounding,
                        uint32_t sign_mask, int sr, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    MxSr s;
    const MxSr *use;
    if (int rc = had_sr_args(sr, seed, offset, &s, &use)) return rc;
    return mxh_launch(kEncode, x, codes, scales, FP8Q_DT_F32, -1, R, K, fmt, rounding, sign_mask, 0, (hipStream_t)stream, use);
}

int fp8q_mxh_encode_h16(const void *x, uint8_t *codes, uint8_t *scales, int x_type, int64_t R, int64_t K, int fmt,
                        int rounding, uint32_t sign_mask, int sr, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    MxSr s;
    const MxSr *use;
    if (int rc = had_sr_args(sr, seed, offset, &s, &use)) return rc;
    return mxh_launch(kEncode, x, codes, scales, x_type, -1, R, K, fmt, rounding, sign_mask, 0, (hipStream_t)stream, use);
}

int fp8q_mxh_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, uint32_t sign_mask, int sr,
                          uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    MxSr s;
    const MxSr *use;
    if (int rc = had_sr_args(sr, seed, offset, &s, &use)) return rc;
    return mxh_launch(kQuant, x, y, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, fmt, rounding, sign_mask, 0, (hipStream_t)stream,
                      use);
}

int fp8q_mxh_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                          uint32_t sign_mask, int sr, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    MxSr s;
    const MxSr *use;
    if (int rc = had_sr_args(sr, seed, offset, &s, &use)) return rc;
    return mxh_launch(kQuant, x, y, nullptr, x_type, y_type, R, K, fmt, rounding, sign_mask, 0, (hipStream_t)stream, use);
}

}  // extern "C"
