// fp8q_ocp.hip -- the hardware FP8 lane (gfx950 only): the OCP encodings E4M3FN and E5M2 that the chip's matrix cores and
// torch.float8_e4m3fn / torch.float8_e5m2 read, made with the chip's own conversion instructions (v_cvt_pk_fp8_f32 /
// v_cvt_pk_bf8_f32, v_cvt_f32_fp8 / v_cvt_f32_bf8).  The emulated formats of the other lanes (a real-valued exponent bias,
// the top exponent code an ordinary binade) cannot be transcoded into these bytes; this lane has its own arithmetic.
//
// Arithmetic contract (include/fp8q.h states it for callers), fmax = 448 (E4M3FN) / 57344 (E5M2):
//   scale = t_max(maxval, eps) / fmax          fp32, IEEE division; a NaN maxval gives a NaN scale
//   q     = t_clamp(x / scale, -fmax, fmax)    fp32 IEEE division, torch.clamp: NaN passes, +-inf saturate
//   code  = RNE(q) as an OCP byte              subnormals as OCP has them, -0 -> 0x80, every NaN -> 0x7F; the clamp comes
//                                              first, so the instruction never sees a value it would overflow on
//   decode(code) = value(code) * scale         one fp32 multiplication; a half output rounds that product once
//   quantize(x)  = decode(encode(x))           the same two device functions in one pass
// The oracle is torch's CPU cast: torch.clamp(x / scale, -fmax, fmax).to(torch.float8_*), and c.float() * scale.
//
// The division.  A lane computes q0 = x * r with r = fl(1 / scale) and converts, not q0, but the two ends of an interval
// that must contain the true quotient qd = fl(x / scale):
//   r = (1/scale)(1 + d1), q0 = (x/scale)(1 + d1)(1 + d2), qd = (x/scale)(1 + d3), |d_i| <= 2^-24, so
//   qd / q0 = (1 + d3) / ((1 + d1)(1 + d2)) lies within 1 +- 3 * 2^-24 (1 + 2^-22)  <  1 +- 2^-22.
//   lo = fl(q0 * (1 - 2^-21)), hi = fl(q0 * (1 + 2^-21)): each product is rounded once (<= 2^-24), so the interval reaches at
//   least q0 (1 +- 7 * 2^-24) on either side -- more than twice the bound above.
// Clamping and RNE are monotonic, so when code(clamp(lo)) == code(clamp(hi)) the quotient, which lies between them, has that
// code as well, and no rounding boundary (a midpoint of two neighbouring FP8 values, subnormal ones included) lies within
// the reciprocal's error of q0.  When the two codes differ such a boundary may lie between q0 and qd -- an exact tie
// x / scale = midpoint always lands here, the interval contains qd strictly -- and the dword's four elements are redone with
// the IEEE division (about 2^-16 of all elements: the interval is 2^-20 wide against an FP8 step of 2^-3 or 2^-2).  Near
// +-fmax both ends clamp to (or round to) fmax: no redo is needed there.  The bounds need normal numbers: a quotient in
// fp32's subnormal range is far below the smallest FP8 midpoint (2^-10 / 2^-17) and becomes a zero of x's sign on both
// routes; scale <= fmax-th of FLT_MAX keeps r normal, and a row whose r overflows (scale below 2^-126) stores r = NaN,
// which sends every element of the row to the division.  NaN products take that route too (the rule below wants them
// told apart anyway).
//
// What the conversion instructions are NOT trusted with, and plain C++ does instead:
//   - NaN.  Encode stores 0x7F for every NaN quotient, whatever its sign or payload.  Decode gives a NaN code (E4M3FN 0x7F /
//     0xFF; E5M2 0x7D..0x7F / 0xFD..0xFF) the bits torch's widening gives it -- sign, quiet bit, the mantissa field left
//     aligned: 0x7FF00000 for E4M3FN 0x7F, 0x7FE00000 / 0x7FC00000 / 0x7FE00000 for E5M2 -- and does not multiply it.
//   - overflow: never reached (the clamp).
// Everything else -- RNE, subnormal results, -0, E5M2's infinities on decode -- is the instruction's.
//
// Kernel: k_ocp<MODE, F, IN, OUT, PC, VEC, NT>, the geometry of the INT codec (fp8q_intq.h: one aligned 4096-element chunk per
// block, chunk_rows() building {scale, 1/scale} of the rows overlapping the chunk in LDS, Chunk::at finding an element's row
// by magic division, so rows of any length -- shorter than 4, longer than a chunk -- need no second path).  Encode: a lane
// owns 16 consecutive elements, its 16-byte loads (four of fp32, two of half) are issued before any arithmetic, and 16 codes
// leave as ONE 16-byte word.  Decode and quantize: lane <-> group of 4 elements (one dword of codes), four groups per lane
// a block apart, so that every store instruction of a wave writes whole lines.  VEC needs both pointers 16-byte aligned
// (host check); anything else, and the elements behind the last group of the last chunk, go element by element.  NT:
// nontemporal loads and stores from 64 MiB (kNtBytes).  The block in whose chunk a row starts writes scale_out[row].  One launch per call, nothing read back.
// HBM traffic per element: encode / decode 5 B (3 B on half tensors), quantize 8 B (4 B half to half).
// Shared with fp8q_mx.hip through fp8q_io.h: the launch modes, the Io* element policies, Fp8Fmt (the conversion instructions)
// and io_dispatch(), the (mode, in_type, out_type) ladder that ocp_launch ends in.
//
// SR (the fp8q_ocpsr_* entries; include/fp8q.h states the draw and the rounding): code = RNE(SR(q, r)) with q by the IEEE
// division for every element (fp8q_ocpq.h says why) and r the 16-bit draw of the element's flat index offset + e.  A chunk
// starts on a multiple of 4096 and offset is a multiple of 8, so an encoding lane's 16 elements are two whole Philox calls
// and a quantizing lane's aligned group of 4 is half a call; the scalar tail and the unaligned route take one call per
// element.  SR = false is the kernel as it was: its argument block is IntArgs, nothing of the draw is compiled in.
#include "fp8q_common.h"
#include "fp8q_intq.h"
#include "fp8q_io.h"
#include "fp8q_ocpq.h"      // the lane's device arithmetic (OcpFmt, ocp_scale_pair, code4 / code1, value4 / value_at): one
                            // copy for this file and fp8q_ocp_block.hip

namespace {

// the row constants {scale, 1/scale} of the encoding side: scale from (maxval, eps), reported where the row starts
template <int F>
struct ScaleOfRange {
    const IntArgs &a;
    __device__ __forceinline__ float4 operator()(int64_t row, bool starts) const
    {
        const float4 k = ocp_scale_pair<F>(a.a[row], a.eps);      // (an overflowing 1/scale is NaN: the row by the division)
        if (starts && a.delta_out) a.delta_out[row] = k.x;
        return k;
    }
};

// ... and of decode: the scale as it was reported
struct ScaleGiven {
    const IntArgs &a;
    __device__ __forceinline__ float4 operator()(int64_t row, bool) const { return make_float4(a.a[row], 0.0f, 0.0f, 0.0f); }
};

// the SR kernels' argument block: IntArgs and the call's seed and offset
struct OcpSrArgs : IntArgs {
    MxSr sr;
};
template <bool SR>
using OcpArgs = std::conditional_t<SR, OcpSrArgs, IntArgs>;

// IntArgs as this lane reads it: a = maxval (decode: scale), delta_out = scale_out or null, eps, the chunk geometry
template <int MODE, int F, class IN, class OUT, bool SR, bool PC, bool VEC, bool NT>
__global__ void __launch_bounds__(kBlock)
k_ocp(const void *__restrict__ in, void *__restrict__ out, OcpArgs<SR> a)
{
    static_assert(!SR || MODE != kDecode, "decode rounds nothing");
    typedef typename IN::elem in_t;
    typedef typename OUT::elem out_t;
    extern __shared__ float4 kc[];
    Chunk c;
    if constexpr (MODE == kDecode) chunk_rows<PC>(c, a, kc, ScaleGiven{a});
    else chunk_rows<PC>(c, a, kc, ScaleOfRange<F>{a});
    const int tid = threadIdx.x;
    const in_t *x = static_cast<const in_t *>(in);
    out_t *y = static_cast<out_t *>(out);
    int64_t tail = c.e0;
    if constexpr (VEC && MODE == kEncode) {
        // both sides 16-byte aligned, e0 a multiple of 4096.  The narrow side is the STORE: a lane owns 16 consecutive
        // elements (a chunk has at most 256 such groups, one per lane) and stores their codes as one 16-byte word
        const int ng = (int)((c.e1 - c.e0) >> 4);
        if (tid < ng) {
            const int off = 16 * tid;
            float v[16];
            IN::template load16<NT>(x + c.e0 + off, v);
            uint32_t w[4];
            uint32_t r[SR ? 16 : 1];
            if constexpr (SR) {
                const uint64_t i0 = a.sr.offset + (uint64_t)(c.e0 + off);       // a multiple of 8
                uint32_t d[8];
                mx_draw8(a.sr, i0, d);
                mx_draw8(a.sr, i0 + 8u, d + 4);
#pragma unroll
                for (int g = 0; g < 4; ++g) mx_split4(d + 2 * g, r + 4 * g);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 k[4] = {c.at<PC>(off + 4 * g), c.at<PC>(off + 4 * g + 1), c.at<PC>(off + 4 * g + 2),
                                     c.at<PC>(off + 4 * g + 3)};
                if constexpr (SR) w[g] = code4_sr<F>(v + 4 * g, k, r + 4 * g);
                else w[g] = code4<F>(v + 4 * g, k);
            }
            stv<NT>(reinterpret_cast<u4v *>(y + c.e0 + off), u4v{w[0], w[1], w[2], w[3]});
        }
        tail = c.e0 + 16 * (int64_t)ng;
    } else if constexpr (VEC) {
        // decode and quantize: the wide side is the store, and a lane that stored its own 64 consecutive bytes left every
        // store instruction of the wave writing a quarter of 64 different lines (measured: 0.9 TB/s).  So the INT decoder's
        // mapping: lane <-> group of 4 elements (one dword of codes), neighbouring lanes neighbouring groups, a full chunk
        // with its four loads in flight, a partial one group by group, the <= 3 elements behind the last group one by one
        const int ngroups = (int)((c.e1 - c.e0) >> 2);
        auto group = [&](const float *v, uint32_t w, int off) {
            const float4 k[4] = {c.at<PC>(off), c.at<PC>(off + 1), c.at<PC>(off + 2), c.at<PC>(off + 3)};
            if constexpr (MODE == kQuant && SR) {
                uint32_t r[4];
                sr_draws4(a.sr, a.sr.offset + (uint64_t)(c.e0 + off), r);
                w = code4_sr<F>(v, k, r);
            } else if constexpr (MODE == kQuant) {
                w = code4<F>(v, k);
            }
            float r[4];
            value4<F>(w, k, r);
            OUT::template store4<NT>(y + c.e0 + off, r);
        };
        if (ngroups == kIntChunk / 4) {
            float v[4][4];
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int off = 4 * (u * kBlock + tid);
                if constexpr (MODE == kDecode) w[u] = IoCodes::load4<NT>(x + c.e0 + off);
                else IN::template load4<NT>(x + c.e0 + off, v[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) group(v[u], w[u], 4 * (u * kBlock + tid));
        } else {
            for (int g = tid; g < ngroups; g += kBlock) {
                float v[4];
                uint32_t w = 0u;
                if constexpr (MODE == kDecode) w = IoCodes::load4<NT>(x + c.e0 + 4 * g);
                else IN::template load4<NT>(x + c.e0 + 4 * g, v);
                group(v, w, 4 * g);
            }
        }
        tail = c.e0 + 4 * (int64_t)ngroups;
    }
    for (int64_t e = tail + tid; e < c.e1; e += kBlock) {
        const float4 k = c.at<PC>((int)(e - c.e0));
        uint32_t code;
        if constexpr (MODE == kDecode) code = x[e];
        else if constexpr (SR) code = code1_sr<F>(IN::load1(x + e), k, mx_draw1(a.sr, a.sr.offset + (uint64_t)e));
        else code = code1<F>(IN::load1(x + e), k);
        if constexpr (MODE == kEncode) y[e] = (uint8_t)code;
        else OUT::store1(y + e, value_at<F, 0>(code, k.x));
    }
}

// scale[i] = t_max(maxval[i], eps) / fmax: what the kernels above use and report, for callers that hold a range only
template <int F>
__global__ void __launch_bounds__(kBlock)
k_ocp_scale(const float *__restrict__ maxval, float *__restrict__ scale, int64_t n, float eps)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) scale[i] = t_max(maxval[i], eps) / OcpFmt<F>::fmax;
}

template <int MODE, int F, class IN, class OUT, bool SR>
void launch_io(const void *in, void *out, const OcpArgs<SR> &a, bool pc, hipStream_t st)
{
    const bool vec = int_vec16(in, out);
    if (pc) FP8Q_INT_LAUNCH(vec, in, out, a, st, k_ocp, MODE, F, IN, OUT, SR, true);
    else FP8Q_INT_LAUNCH(vec, in, out, a, st, k_ocp, MODE, F, IN, OUT, SR, false);
}

// Argument checks (everything is reported before the launch) and the one launch.  in_type / out_type: FP8Q_DT_* of the value
// side(s), -1 for the side that holds codes.  range: maxval, or decode's scale.  sr: the seed and offset of a
// stochastic-rounding entry (encode, quantize), null for round to nearest even.
int ocp_launch(int mode, const void *in, void *out, int in_type, int out_type, int64_t C, int64_t inner, const float *range,
               int64_t n_range, int fmt, float eps, float *scale_out, hipStream_t st, const MxSr *sr = nullptr)
{
    if (int rc = int_check_x(in, out, C, inner, n_range)) return rc;
    if (!range) return FP8Q_EINVAL;
    if (fmt != FP8Q_OCP_E4M3FN && fmt != FP8Q_OCP_E5M2) return FP8Q_EUNSUPPORTED;
    if (value_side_misaligned(in, in_type) || value_side_misaligned(out, out_type) || ((uintptr_t)range & 3) ||
        ((uintptr_t)scale_out & 3))
        return FP8Q_EINVAL;
    if (sr && (sr->offset & 7u)) return FP8Q_EINVAL;
    const bool pc = n_range > 1;
    OcpSrArgs a = {};
    a.a = range;
    a.eps = eps;
    a.delta_out = scale_out;
    a.C = n_range;
    if (sr) a.sr = *sr;
    int_geometry(a, C, inner, pc);
    io_dispatch(mode, in_type, out_type, [&](auto m, auto ti, auto to) {
        constexpr int MODE = decltype(m)::value;
        typedef decltype(ti) IN;
        typedef decltype(to) OUT;
        auto go = [&](auto sr_on) {
            constexpr bool SR = decltype(sr_on)::value;
            const OcpArgs<SR> &as = a;          // (the round-to-nearest-even kernels take the IntArgs part)
            if (fmt == FP8Q_OCP_E4M3FN) launch_io<MODE, FP8Q_OCP_E4M3FN, IN, OUT, SR>(in, out, as, pc, st);
            else launch_io<MODE, FP8Q_OCP_E5M2, IN, OUT, SR>(in, out, as, pc, st);
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

int fp8q_ocp_encode_f32(const float *x, uint8_t *codes, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                        int fmt, float eps, float *scale_out, fp8q_stream_t stream)
{
    return ocp_launch(kEncode, x, codes, FP8Q_DT_F32, -1, C, inner, maxval, n_maxval, fmt, eps, scale_out, (hipStream_t)stream);
}

int fp8q_ocp_encode_h16(const void *x, uint8_t *codes, int x_type, int64_t C, int64_t inner, const float *maxval,
                        int64_t n_maxval, int fmt, float eps, float *scale_out, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    return ocp_launch(kEncode, x, codes, x_type, -1, C, inner, maxval, n_maxval, fmt, eps, scale_out, (hipStream_t)stream);
}

int fp8q_ocp_decode_f32(const uint8_t *codes, float *y, int64_t C, int64_t inner, const float *scale, int64_t n_scale, int fmt,
                        fp8q_stream_t stream)
{
    return ocp_launch(kDecode, codes, y, -1, FP8Q_DT_F32, C, inner, scale, n_scale, fmt, 0.0f, nullptr, (hipStream_t)stream);
}

int fp8q_ocp_decode_h16(const uint8_t *codes, void *y, int y_type, int64_t C, int64_t inner, const float *scale,
                        int64_t n_scale, int fmt, fp8q_stream_t stream)
{
    if (!half_type(y_type)) return FP8Q_EINVAL;
    return ocp_launch(kDecode, codes, y, -1, y_type, C, inner, scale, n_scale, fmt, 0.0f, nullptr, (hipStream_t)stream);
}

int fp8q_ocp_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval, int fmt,
                          float eps, fp8q_stream_t stream)
{
    return ocp_launch(kQuant, x, y, FP8Q_DT_F32, FP8Q_DT_F32, C, inner, maxval, n_maxval, fmt, eps, nullptr,
                      (hipStream_t)stream);
}

int fp8q_ocp_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *maxval,
                          int64_t n_maxval, int fmt, float eps, fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    return ocp_launch(kQuant, x, y, x_type, y_type, C, inner, maxval, n_maxval, fmt, eps, nullptr, (hipStream_t)stream);
}

int fp8q_ocpsr_encode_f32(const float *x, uint8_t *codes, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                          int fmt, float eps, float *scale_out, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return ocp_launch(kEncode, x, codes, FP8Q_DT_F32, -1, C, inner, maxval, n_maxval, fmt, eps, scale_out, (hipStream_t)stream,
                      &sr);
}

int fp8q_ocpsr_encode_h16(const void *x, uint8_t *codes, int x_type, int64_t C, int64_t inner, const float *maxval,
                          int64_t n_maxval, int fmt, float eps, float *scale_out, uint64_t seed, uint64_t offset,
                          fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    const MxSr sr = mx_sr_args(seed, offset);
    return ocp_launch(kEncode, x, codes, x_type, -1, C, inner, maxval, n_maxval, fmt, eps, scale_out, (hipStream_t)stream, &sr);
}

int fp8q_ocpsr_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval, int fmt,
                            float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return ocp_launch(kQuant, x, y, FP8Q_DT_F32, FP8Q_DT_F32, C, inner, maxval, n_maxval, fmt, eps, nullptr,
                      (hipStream_t)stream, &sr);
}

int fp8q_ocpsr_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *maxval,
                            int64_t n_maxval, int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    const MxSr sr = mx_sr_args(seed, offset);
    return ocp_launch(kQuant, x, y, x_type, y_type, C, inner, maxval, n_maxval, fmt, eps, nullptr, (hipStream_t)stream, &sr);
}

int fp8q_ocp_scale_f32(const float *maxval, int64_t n, int fmt, float eps, float *scale, fp8q_stream_t stream)
{
    if (!maxval || !scale || n <= 0 || (((uintptr_t)maxval | (uintptr_t)scale) & 3)) return FP8Q_EINVAL;
    if (fmt != FP8Q_OCP_E4M3FN && fmt != FP8Q_OCP_E5M2) return FP8Q_EUNSUPPORTED;
    if (cdiv(n, kBlock) > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    const dim3 g((unsigned)cdiv(n, kBlock)), b(kBlock);
    if (fmt == FP8Q_OCP_E4M3FN)
        hipLaunchKernelGGL((k_ocp_scale<FP8Q_OCP_E4M3FN>), g, b, 0, (hipStream_t)stream, maxval, scale, n, eps);
    else
        hipLaunchKernelGGL((k_ocp_scale<FP8Q_OCP_E5M2>), g, b, 0, (hipStream_t)stream, maxval, scale, n, eps);
    return launch_rc();
}

}  // extern "C"
