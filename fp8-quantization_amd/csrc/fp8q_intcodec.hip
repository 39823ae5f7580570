// fp8q_intcodec.hip -- the storage form of the uniform (INT) quantizers: the integers themselves.
//
// Extends the arithmetic contract at the top of fp8q_int.hip (scale, zp, int_min, int_max exactly as consts_of() and
// k_int_quant form them, the symmetric sign read from device memory):
//   t = clamp(rint(x / scale) + zp, int_min, int_max)      int_level(), fp8q_intq.h: fp32, every op rounded on its own
//   to_integer  t as float32.  NaN stays NaN; -0 + zp is what fp32 gives.  A zero level is stored as +0, as the CUDA chain
//               stores it: the only -0 the formula can yield is clamp(-0 + -0, 0, hi) of an asymmetric range whose
//               zero_float is -0 (x_min >= +0), and torch's CUDA clamp computes max(-0, +0), which is +0 on the GPU
//               (its CPU clamp keeps the -0: the one place where the two torch chains differ here).
//   encode      t as an integer: one byte for n_bits <= 8, two bytes (little endian) for 9..16, the two's-complement low
//               bits of t -- unsigned ranges store 0 .. 2^n - 1, the signed symmetric range -2^(n-1) .. 2^(n-1) - 1.
//               NaN has no code: it stores the code of the value 0, which is zp (asymmetric) or 0 (symmetric), as the FP8
//               encoder stores 0; a channel whose zp is NaN itself (zero_float NaN) stores 0.
//   decode      y = scale * (float(code) - zp), the code read as signed exactly when the quantizer is symmetric and its
//               device sign flag is set.
// Consequences:
//   decode(encode(x)) == fp8q_int_quantize_f32(x) bit for bit on every element whose x is not NaN, +-inf inputs and
//   channels with delta 0 / inf / NaN included: both run the same last two operations on the same exactly representable
//   integer (the sign of a zero t does not reach y: t - zp is +0 whenever they are equal).
//   encode(x) == to_integer(x) cast to the storage type wherever to_integer(x) is not NaN.
//   to_integer(x) == the eager to_integer_forward chain bit for bit on the same range buffers.
//
// Kernels -- k_int_quant's geometry: one aligned 4096-element chunk per block, the channel constants {scale, 1/scale, zp}
// of the rows overlapping the chunk built once per block in LDS, the channel of an element from the magic division.  The
// argument block, that prologue (chunk_setup), k_int_level's streaming loop (chunk_walk) and the host side of the launch
// are fp8q_intq.h's, shared with fp8q_int.hip, as are int_fixed_args() and the code dwords (pack_codes / code_at, also used
// by fp8q_codec_h16.hip); encode and decode keep their own group shapes:
//   k_int_encode<W, PC, VEC, NT>  the wide side is the LOAD: a lane owns 16 (W = 1) or 8 (W = 2) consecutive elements,
//                 issues its four 16-byte loads before any arithmetic and stores the codes as ONE 16-byte word.
//   k_int_decode<W, PC, VEC, NT>  the wide side is the STORE (the FP8 decoder's mapping): lane <-> 4-element group, one
//                 4-byte (W = 1) or 8-byte (W = 2) word of codes per group, whole aligned 16-byte fp32 stores.
//   k_int_level<PC, VEC, NT>      k_int_quant's streaming, storing t.
// VEC needs both sides aligned to their vector word (host check); anything else, and the ragged tail of the last chunk,
// goes element by element.  One launch per call, no workspace, nothing read back.
// HBM traffic: encode / decode 5 B per element (6 B with 2-byte codes), to_integer 8 B.
#include "fp8q_common.h"
#include "fp8q_half.h"
#include "fp8q_intq.h"

namespace {

// a code, and the word of a 4-element group's codes (u2v / u4v: fp8q_half.h)
template <int W>
struct CodeType {
    typedef uint8_t type;
    typedef uint32_t word;
};
template <>
struct CodeType<2> {
    typedef uint16_t type;
    typedef u2v word;
};

template <int W, bool PC, bool VEC, bool NT>
__global__ void __launch_bounds__(kBlock)
k_int_encode(const void *__restrict__ in, void *__restrict__ codes, IntArgs a)
{
    typedef typename CodeType<W>::type code_t;
    const float *__restrict__ x = static_cast<const float *>(in);
    constexpr uint32_t kMask = W == 1 ? 0xffu : 0xffffu;
    extern __shared__ float4 kc[];
    const int tid = threadIdx.x;
    const Chunk c = chunk_setup<PC>(a, kc, ReadRange{a});
    const int64_t e0 = c.e0, e1 = c.e1;
    code_t *out = static_cast<code_t *>(codes);
    int64_t tail = e0;
    if (VEC) {
        // x and codes 16-byte aligned, e0 a multiple of 4096: a group is EPG elements = LPG loads = one 16-byte code word
        constexpr int EPG = 16 / W, LPG = EPG / 4, GPL = kIntChunk / EPG / kBlock;
        const int ngroups = (int)((e1 - e0) / EPG);
        const vf4 *xv = reinterpret_cast<const vf4 *>(x + e0);
        u4v *cv = reinterpret_cast<u4v *>(out + e0);
        auto pack = [&](const vf4 *v, int off) -> u4v {
            uint32_t q[EPG];
#pragma unroll
            for (int j = 0; j < LPG; ++j) {
                q[4 * j] = code_of(v[j].x, c.at<PC>(off + 4 * j), c.lo, c.hi) & kMask;
                q[4 * j + 1] = code_of(v[j].y, c.at<PC>(off + 4 * j + 1), c.lo, c.hi) & kMask;
                q[4 * j + 2] = code_of(v[j].z, c.at<PC>(off + 4 * j + 2), c.lo, c.hi) & kMask;
                q[4 * j + 3] = code_of(v[j].w, c.at<PC>(off + 4 * j + 3), c.lo, c.hi) & kMask;
            }
            return u4v{pack_codes<W>(q), pack_codes<W>(q + 4 / W), pack_codes<W>(q + 8 / W), pack_codes<W>(q + 12 / W)};
        };
        if (ngroups == kIntChunk / EPG) {
            vf4 v[GPL * LPG];
#pragma unroll
            for (int u = 0; u < GPL; ++u)
#pragma unroll
                for (int j = 0; j < LPG; ++j) v[u * LPG + j] = ldv<NT>(xv + (u * kBlock + tid) * LPG + j);
#pragma unroll
            for (int u = 0; u < GPL; ++u) stv<NT>(cv + u * kBlock + tid, pack(v + u * LPG, (u * kBlock + tid) * EPG));
        } else {
            for (int g = tid; g < ngroups; g += kBlock) {
                vf4 v[LPG];
#pragma unroll
                for (int j = 0; j < LPG; ++j) v[j] = ldv<NT>(xv + g * LPG + j);
                stv<NT>(cv + g, pack(v, g * EPG));
            }
        }
        tail = e0 + (int64_t)ngroups * EPG;
    }
    for (int64_t e = tail + tid; e < e1; e += kBlock)
        out[e] = (code_t)code_of(x[e], c.at<PC>((int)(e - e0)), c.lo, c.hi);
}

template <int W, bool PC, bool VEC, bool NT>
__global__ void __launch_bounds__(kBlock)
k_int_decode(const void *__restrict__ codes, void *__restrict__ out, IntArgs a)
{
    float *__restrict__ y = static_cast<float *>(out);
    typedef typename CodeType<W>::type code_t;
    extern __shared__ float4 kc[];
    const int tid = threadIdx.x;
    const Chunk c = chunk_setup<PC>(a, kc, ReadRange{a});
    const int64_t e0 = c.e0, e1 = c.e1;
    const code_t *in = static_cast<const code_t *>(codes);
    int64_t tail = e0;
    if (VEC) {
        // y 16-byte aligned, codes aligned to a group's word (4 W bytes), e0 a multiple of 4096
        typedef typename CodeType<W>::word word_t;
        const int ngroups = (int)((e1 - e0) >> 2);
        const word_t *cw = reinterpret_cast<const word_t *>(in + e0);
        vf4 *yv = reinterpret_cast<vf4 *>(y + e0);
        auto unpack = [&](const word_t w, int off) -> vf4 {
            uint32_t q[4];
            if constexpr (W == 1) {
                q[0] = code_at<1>(w, 0), q[1] = code_at<1>(w, 1), q[2] = code_at<1>(w, 2), q[3] = code_at<1>(w, 3);
            } else {
                q[0] = code_at<2>(w.x, 0), q[1] = code_at<2>(w.x, 1), q[2] = code_at<2>(w.y, 0), q[3] = code_at<2>(w.y, 1);
            }
            return vf4{value_of<W>(q[0], c.sgn, c.at<PC>(off)), value_of<W>(q[1], c.sgn, c.at<PC>(off + 1)),
                       value_of<W>(q[2], c.sgn, c.at<PC>(off + 2)), value_of<W>(q[3], c.sgn, c.at<PC>(off + 3))};
        };
        if (ngroups == kIntChunk / 4) {
            word_t w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = ldv<NT>(cw + u * kBlock + tid);
#pragma unroll
            for (int u = 0; u < 4; ++u) st16<NT>(yv + u * kBlock + tid, unpack(w[u], 4 * (u * kBlock + tid)));
        } else {
            for (int g = tid; g < ngroups; g += kBlock) st16<NT>(yv + g, unpack(ldv<NT>(cw + g), 4 * g));
        }
        tail = e0 + 4 * (int64_t)ngroups;
    }
    for (int64_t e = tail + tid; e < e1; e += kBlock) y[e] = value_of<W>(in[e], c.sgn, c.at<PC>((int)(e - e0)));
}

// to_integer's element: the level, a zero as +0 (see the contract above; x + 0 changes nothing else, NaN included)
__device__ __forceinline__ float level_of(float v, const float4 k, float lo, float hi)
{
    return int_level(v, k, lo, hi) + 0.0f;
}

template <bool PC, bool VEC, bool NT>
__global__ void __launch_bounds__(kBlock)
k_int_level(const void *__restrict__ in, void *__restrict__ out, IntArgs a)
{
    extern __shared__ float4 kc[];
    chunk_walk<PC, VEC, NT, level_of>(static_cast<const float *>(in), static_cast<float *>(out),
                                      chunk_setup<PC>(a, kc, ReadRange{a}));
}

enum { kEncode, kDecode, kLevel };

// argument checks (those of fp8q_int_quantize_f32) and the one launch; `in` / `out`: x -> codes, codes -> y, x -> t
int codec_launch(int mode, const void *in, void *out, int64_t C, int64_t inner, const float *delta,
                 const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits, int symmetric,
                 float eps, hipStream_t st)
{
    if (int rc = int_check_x(in, out, C, inner, n_delta)) return rc;
    IntArgs a = {};
    if (int rc = int_fixed_args(a, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps)) return rc;
    const int W = n_bits <= 8 ? 1 : 2;
    const uintptr_t pin = (uintptr_t)in, pout = (uintptr_t)out;
    if (((mode == kDecode ? pout : pin) & 3) || (mode == kLevel && (pout & 3))) return FP8Q_EINVAL;   // fp32 sides
    if (mode != kLevel && ((mode == kEncode ? pout : pin) & (uintptr_t)(W - 1))) return FP8Q_EINVAL;   // codes
    const bool pc = n_delta > 1;
    int_geometry(a, C, inner, pc);
    // both sides on their vector word: 16 bytes, or (decode) a group's 4 W bytes of codes
    const bool vec = mode == kDecode ? ((pout & 15) == 0 && (pin & (uintptr_t)(4 * W - 1)) == 0) : int_vec16(in, out);
    if (mode == kLevel) {
        if (pc) FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_level, true);
        else FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_level, false);
    } else if (mode == kEncode) {
        if (W == 1 && pc) FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_encode, 1, true);
        else if (W == 1) FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_encode, 1, false);
        else if (pc) FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_encode, 2, true);
        else FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_encode, 2, false);
    } else {
        if (W == 1 && pc) FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_decode, 1, true);
        else if (W == 1) FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_decode, 1, false);
        else if (pc) FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_decode, 2, true);
        else FP8Q_INT_LAUNCH(vec, in, out, a, st, k_int_decode, 2, false);
    }
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_int_to_integer_f32(const float *x, float *t, int64_t C, int64_t inner, const float *delta,
                            const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                            int symmetric, float eps, fp8q_stream_t stream)
{
    return codec_launch(kLevel, x, t, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps,
                        (hipStream_t)stream);
}

int fp8q_int_encode(const float *x, void *codes, int64_t C, int64_t inner, const float *delta, const float *zero_float,
                    int64_t n_delta, const unsigned char *signed_flag, int n_bits, int symmetric, float eps,
                    fp8q_stream_t stream)
{
    return codec_launch(kEncode, x, codes, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps,
                        (hipStream_t)stream);
}

int fp8q_int_decode(const void *codes, float *y, int64_t C, int64_t inner, const float *delta, const float *zero_float,
                    int64_t n_delta, const unsigned char *signed_flag, int n_bits, int symmetric, float eps,
                    fp8q_stream_t stream)
{
    return codec_launch(kDecode, codes, y, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps,
                        (hipStream_t)stream);
}

}  // extern "C"
