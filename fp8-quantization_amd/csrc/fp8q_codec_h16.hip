// fp8q_codec_h16.hip -- the storage codes of the half-precision lane (gfx950 only): FP8 codes (fp8q_codec.hip's) and INT
// codes (fp8q_intcodec.hip's) straight from and to IEEE fp16 / bfloat16 tensors.  Element type selected at run time (x_type /
// y_type = FP8Q_DT_F16 / FP8Q_DT_BF16, include/fp8q.h).
//
// Arithmetic contract:
//   - every half input is widened to fp32 EXACTLY, as fp8q_h16.hip does it (fp8q_half.h): fp16 subnormals become normal
//     fp32 numbers, bf16 is the upper half of an fp32 word, nothing is flushed.  From there the fp32 code runs unchanged,
//     through the same device functions: make_chan / lut_part / lut_entry, encode_group4 / encode_one / decode_one
//     (fp8q_device.h), consts_of / int_level / code_of / value_of (fp8q_intq.h, the reciprocal-then-redo rule included).
//   - fp8q_encode_h16(x) == fp8q_encode_u8(widen(x)) byte for byte; NaN inputs and degenerate channels (maxval 0 / inf /
//     NaN) encode as 0.  fp8q_int_encode_h16(x) == fp8q_int_encode(widen(x)): one byte for n_bits <= 8, two bytes (little
//     endian) for 9..16, the same NaN and sign rules.
//   - fp8q_decode_h16 / fp8q_int_decode_h16 take the fp32 value of fp8q_decode_u8 / fp8q_int_decode and round it ONCE to
//     y_type, round to nearest even, overflow to infinity (what torch.Tensor.to(dtype) does).  That fp32 value exists
//     before it is narrowed: F16::narrow1 / narrow2 hold it in a register of its own, so the last multiplication and the
//     conversion are never fused into one rounding (v_fma_mixlo_f16).
//   - hence decode_h16(encode_h16(x), T) == fp8q_quantize_h16(x, y_type = T) wherever the fp32 round trip equals K1 (the
//     geometric-scale condition stated for fp8q_decode_u8: all weight-sized ranges), and for INT wherever x is not NaN.
//
// Kernels (every entry point is one launch):
//   k_h16_encode<T, PC, U>   k_h16_quant's flat cut: the (<= 7) elements up to x's 16-byte boundary and the (<= 15) behind
//                       the last whole group are scalars of block 0; the body is cut into chunks of 256 * U groups of 16
//                       elements.  A lane owns a group: two consecutive 16-byte loads, issued before the {s, 1/s} tables
//                       of the rows overlapping the chunk are built in LDS, and ONE 16-byte store of 16 codes when the
//                       codes share the body's phase against the 16-byte grid (four dwords at a 4-byte phase, bytes
//                       otherwise: a narrow code store per group was the fp32 encoder's limit, docs/HISTORY.md N3).  Each
//                       half of a group may straddle a row border (rows of >= 8 elements: at most two rows per 8 elements);
//                       every element takes the constants and the table of its own row (TwoRows), as quant_group_2rows does.
//   k_h16_decode<T, PC, U>   the cut is the CODES': up to 15 scalars in front of their 16-byte boundary, then one 16-byte
//                       load of 16 codes and two 16-byte half stores per lane (at the 2-byte phase y happens to have).
//                       The scales of the rows overlapping the chunk sit in LDS; a group that straddles a row border
//                       decodes element-wise with each row's own table (rows of >= 8 elements: at most three rows).
//   k_h16_codec_rows<T, ENCODE>   what the chunk kernels do not take (per-channel rows shorter than 8 elements, rows so
//                       short that the tables of a chunk outgrow LDS): thread = row, no table (encode_direct /
//                       decode_direct: the table's own entry computed on the spot).
//   k_h16_int_encode<T, W, PC> / k_h16_int_decode<T, W, PC>   k_inth16_quant's geometry: one 4096-element chunk per block,
//                       chunk_setup() of fp8q_intq.h as it is, every element with the constants of its own row
//                       (Chunk::at), so rows of any length need no second path.  The scalars of a chunk are those in
//                       front of the wide side's 16-byte boundary (x for encode, the codes for decode) and behind the last
//                       whole group of 16 elements; a lane owns a group: two 16-byte loads of halves -> 16 bytes (W = 1)
//                       or 2 x 16 bytes (W = 2) of codes, and W 16-byte loads of codes -> two 16-byte half stores.
// Only plain vector loads and stores, none nontemporal.  The one size-selected variant is U = 2 of the two FP8 chunk kernels
// (8192-element chunks from 2^19 groups on, when the tables of such a chunk fit the LDS budget).
// HBM traffic per element: 3 B each way (2 B of half + 1 B of code), 4 B with 2-byte INT codes.
#include "fp8q_common.h"
#include "fp8q_half.h"
#include "fp8q_intq.h"

namespace {

// ---------------------------------------------------------------------------------------------
// what the kernels share (widen8, store_half8, scalar_of: fp8q_half.h): the store of a lane's 16 one-byte codes
// ---------------------------------------------------------------------------------------------
// how the 16 one-byte codes of a lane go out (decided on the host from the address of the first group)
enum { kStore16 = 0, kStore4 = 1, kStore1 = 2 };

inline int code_store_of(const void *first_group)
{
    const uintptr_t p = (uintptr_t)first_group;
    return (p & 15) == 0 ? kStore16 : ((p & 3) == 0 ? kStore4 : kStore1);
}

__device__ __forceinline__ void store_codes16(uint8_t *p, const uint32_t (&w)[4], int cs)
{
    if (cs == kStore16) {
        *reinterpret_cast<u4v *>(p) = u4v{w[0], w[1], w[2], w[3]};
    } else if (cs == kStore4) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = w[j];
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

// ---------------------------------------------------------------------------------------------
// FP8 codes
// ---------------------------------------------------------------------------------------------
// encode_group4_of's rows (fp8q_device.h) for four elements of which b.. belong to a second channel (b <= 0: all, b >= 4:
// none): constants and table selected per element, as quant_group_2rows does
struct TwoRows {
    int b;
    const ChanLite &ca, &cb;
    const float2 *la, *lb;
    __device__ __forceinline__ bool always_exact() const { return (b > 0 && ca.pthr < 0.0f) | (b < 4 && cb.pthr < 0.0f); }
    __device__ __forceinline__ ChanLite chan(int j) const
    {
        const bool nx = j >= b;
        ChanLite c;
        c.maxv = nx ? cb.maxv : ca.maxv;
        c.minv = nx ? cb.minv : ca.minv;
        c.bias = nx ? cb.bias : ca.bias;
        c.pthr = nx ? cb.pthr : ca.pthr;
        return c;
    }
    __device__ __forceinline__ const float2 *lut(int j) const { return j >= b ? lb : la; }
};

struct CodecArgs {
    int64_t n;         // elements of the tensor
    int64_t head;      // scalars in front of the wide side's 16-byte boundary (encode: x, <= 7; decode: the codes, <= 15)
    int64_t ng;        // 16-element groups of the body
    int64_t inner;     // row length (per channel), n otherwise
    uint32_t magic;    // o / inner for chunk-local offsets (rows shorter than a chunk)
    int lut_stride;    // pmax + 1
    int nc_max;        // rows a chunk can overlap: LDS entries
    int cs;            // encode: kStore*
    int n_bits;
};

constexpr size_t kCodecLdsBudget = 40 * 1024;   // tables of one chunk

// what a block knows about the rows of its chunk once chunk_tables() has run
struct ChunkRows {
    float4 *chl;       // {maxv, minv, bias, pthr} per row
    float2 *lut;       // {s, 1/s} tables, lut_stride entries per row
    int phase, nrows;
};

// the constants and tables of the rows overlapping the 16 * gn elements from e0 on: four lanes per row share a table
template <bool PC>
__device__ __forceinline__ ChunkRows chunk_tables(unsigned char *smem, const float *__restrict__ maxval, const QFmt &f,
                                                  const CodecArgs &a, int64_t e0, int gn)
{
    ChunkRows r;
    r.chl = reinterpret_cast<float4 *>(smem);
    r.lut = reinterpret_cast<float2 *>(r.chl + a.nc_max);
    int64_t row_lo = 0;
    r.phase = 0;
    r.nrows = 1;
    if (PC) {
        row_lo = e0 / a.inner;
        r.phase = (int)(e0 - row_lo * a.inner);
        r.nrows = (int)(((int64_t)r.phase + 16 * gn - 1) / a.inner) + 1;
    }
    for (int t = threadIdx.x; t < r.nrows * 4; t += kBlock) {
        const int lr = t >> 2, sub = t & 3;
        const Chan c = make_chan(maxval[PC ? row_lo + lr : 0], f);
        if (sub == 0) r.chl[lr] = make_float4(c.maxv, c.minv, c.bias, c.pthr);
        lut_part(r.lut + lr * a.lut_stride, c, f, sub, 4);
    }
    __syncthreads();
    return r;
}

// the chunk-local row of offset o (from the first row's start), and how many elements that row has left from o on
template <int CH>
__device__ __forceinline__ int row_of(uint32_t o, const CodecArgs &a, int &left)
{
    const int lr = a.inner >= CH ? (int)((int64_t)o >= a.inner) : div_small(o, a.magic);
    left = (int)(a.inner - ((int64_t)o - (int64_t)lr * a.inner));   // >= 1
    return lr;
}

template <class T, bool PC, int U>
__global__ void __launch_bounds__(kBlock)
k_h16_encode(const uint16_t *__restrict__ x, uint8_t *__restrict__ codes, const float *__restrict__ maxval, QFmt f, CodecArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int CH = kBlock * 16 * U;
    const int tid = threadIdx.x;
    const float pmaxf = (float)f.pmax;
    const int M = (int)f.M, sign_shift = f.sign_bits == 1 ? a.n_bits - 1 : -1;

    // the body's loads first: the table build below hides their latency
    const int64_t g0 = (int64_t)blockIdx.x * (kBlock * U);
    const int gn = (int)(a.ng - g0 < kBlock * U ? a.ng - g0 : kBlock * U);    // groups of this chunk (0: a tensor without a body)
    const int64_t e0 = a.head + 16 * g0;
    const u4v *xv = reinterpret_cast<const u4v *>(x + e0);
    u4v v[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int q = tid + u * kBlock;
        if (q < gn) {
            v[u][0] = xv[2 * q];
            v[u][1] = xv[2 * q + 1];
        }
    }

    if (blockIdx.x == 0) {   // the scalars around the body: no table
        const int64_t e = scalar_of(tid, a.head, a.head + 16 * a.ng, a.n);
        if (e >= 0) {
            const Chan c = make_chan(maxval[PC ? e / a.inner : 0], f);
            codes[e] = (uint8_t)encode_direct(T::widen1(x[e]), c, f, sign_shift);
        }
    }
    if (gn <= 0) return;
    const ChunkRows r = chunk_tables<PC>(smem, maxval, f, a, e0, gn);

#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int q = tid + u * kBlock;
        if (q >= gn) break;
        uint32_t w[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float e[8];
            widen8<T>(v[u][h], e);
            const float lo4[4] = {e[0], e[1], e[2], e[3]}, hi4[4] = {e[4], e[5], e[6], e[7]};
            if (PC) {
                // e[b..7] belong to the next row (rows hold >= 8 elements: exactly one more row)
                int b;
                const int lr = row_of<CH>((uint32_t)r.phase + 16u * (uint32_t)q + 8u * (uint32_t)h, a, b);
                const int lrn = lr + 1 < r.nrows ? lr + 1 : lr;
                const ChanLite ca = lite_of(r.chl[lr]), cb = lite_of(r.chl[lrn]);
                const float2 *la = r.lut + lr * a.lut_stride, *lb = r.lut + lrn * a.lut_stride;
                w[2 * h] = encode_group4_of(lo4, TwoRows{b, ca, cb, la, lb}, pmaxf, f.qthr, M, sign_shift);
                w[2 * h + 1] = encode_group4_of(hi4, TwoRows{b - 4, ca, cb, la, lb}, pmaxf, f.qthr, M, sign_shift);
            } else {
                const ChanLite c = lite_of(r.chl[0]);
                w[2 * h] = encode_group4(lo4, c, r.lut, pmaxf, f.qthr, M, sign_shift);
                w[2 * h + 1] = encode_group4(hi4, c, r.lut, pmaxf, f.qthr, M, sign_shift);
            }
        }
        store_codes16(codes + e0 + 16 * (int64_t)q, w, a.cs);
    }
}

template <class T, bool PC, int U>
__global__ void __launch_bounds__(kBlock)
k_h16_decode(const uint8_t *__restrict__ codes, uint16_t *__restrict__ y, const float *__restrict__ maxval, QFmt f, CodecArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int CH = kBlock * 16 * U;
    const int tid = threadIdx.x;
    const int M = (int)f.M, sign_shift = f.sign_bits == 1 ? a.n_bits - 1 : -1;

    const int64_t g0 = (int64_t)blockIdx.x * (kBlock * U);
    const int gn = (int)(a.ng - g0 < kBlock * U ? a.ng - g0 : kBlock * U);
    const int64_t e0 = a.head + 16 * g0;
    const u4v *cv = reinterpret_cast<const u4v *>(codes + e0);
    u4v v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (tid + u * kBlock < gn) v[u] = cv[tid + u * kBlock];

    if (blockIdx.x == 0) {
        const int64_t e = scalar_of(tid, a.head, a.head + 16 * a.ng, a.n);
        if (e >= 0) {
            const Chan c = make_chan(maxval[PC ? e / a.inner : 0], f);
            y[e] = T::narrow1(decode_direct(codes[e], c, f.M, sign_shift));
        }
    }
    if (gn <= 0) return;
    const ChunkRows r = chunk_tables<PC>(smem, maxval, f, a, e0, gn);

#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int q = tid + u * kBlock;
        if (q >= gn) break;
        const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        int lr = 0, b = 16;
        if (PC) lr = row_of<CH>((uint32_t)r.phase + 16u * (uint32_t)q, a, b);
        const float2 *lt = r.lut + lr * a.lut_stride;
        float e[16];
        if (!PC || b >= 16) {
#pragma unroll
            for (int j = 0; j < 16; ++j) e[j] = decode_one((w[j >> 2] >> (8 * (j & 3))) & 255u, lt, M, sign_shift);
        } else {
            // the group straddles a row border: rows hold >= 8 elements, so at most two more rows begin in it
            const int b2 = b + (int)(a.inner < 16 ? a.inner : 16);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int lj = (j >= b) + (j >= b2);
                e[j] = decode_one((w[j >> 2] >> (8 * (j & 3))) & 255u, lt + lj * a.lut_stride, M, sign_shift);
            }
        }
        uint16_t *yo = y + e0 + 16 * (int64_t)q;
        store_half8<T>(yo, e);
        store_half8<T>(yo + 8, e + 8);
    }
}

// thread = row, no table: per-channel rows the chunk kernels do not take
template <class T, bool ENCODE>
__global__ void __launch_bounds__(kBlock)
k_h16_codec_rows(const void *__restrict__ in, void *__restrict__ out, int64_t C, int64_t inner, const float *__restrict__ maxval,
                 QFmt f, int n_bits)
{
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= C) return;
    const int sign_shift = f.sign_bits == 1 ? n_bits - 1 : -1;
    const Chan c = make_chan(maxval[row], f);
    for (int64_t j = 0; j < inner; ++j) {
        const int64_t e = row * inner + j;
        if (ENCODE)
            static_cast<uint8_t *>(out)[e] = (uint8_t)encode_direct(T::widen1(static_cast<const uint16_t *>(in)[e]), c, f, sign_shift);
        else
            static_cast<uint16_t *>(out)[e] = T::narrow1(decode_direct(static_cast<const uint8_t *>(in)[e], c, f.M, sign_shift));
    }
}

template <class T, bool ENCODE, bool PC>
void fp8_launch_u(int u, dim3 g, size_t shmem, hipStream_t st, const void *in, void *out, const float *maxval, const QFmt &f,
                  const CodecArgs &a)
{
    if (ENCODE) {
        const uint16_t *x = static_cast<const uint16_t *>(in);
        uint8_t *codes = static_cast<uint8_t *>(out);
        if (u == 1) hipLaunchKernelGGL((k_h16_encode<T, PC, 1>), g, dim3(kBlock), shmem, st, x, codes, maxval, f, a);
        else hipLaunchKernelGGL((k_h16_encode<T, PC, 2>), g, dim3(kBlock), shmem, st, x, codes, maxval, f, a);
    } else {
        const uint8_t *codes = static_cast<const uint8_t *>(in);
        uint16_t *y = static_cast<uint16_t *>(out);
        if (u == 1) hipLaunchKernelGGL((k_h16_decode<T, PC, 1>), g, dim3(kBlock), shmem, st, codes, y, maxval, f, a);
        else hipLaunchKernelGGL((k_h16_decode<T, PC, 2>), g, dim3(kBlock), shmem, st, codes, y, maxval, f, a);
    }
}

// in -> out: x -> codes (ENCODE) or codes -> y
template <class T, bool ENCODE>
int fp8_launch(const void *in, void *out, int64_t C, int64_t inner, const float *maxval, bool pc, const QFmt &f, int n_bits,
               hipStream_t st)
{
    CodecArgs a;
    a.n = C * inner;
    // the cut follows the side that is LOADED 16 bytes at a time: halves (encode) or codes (decode)
    a.head = ENCODE ? (int64_t)(((16 - ((uintptr_t)in & 15)) & 15) >> 1) : (int64_t)((16 - ((uintptr_t)in & 15)) & 15);
    if (a.head > a.n) a.head = a.n;
    a.ng = (a.n - a.head) >> 4;
    a.inner = pc ? inner : a.n;
    a.lut_stride = f.pmax + 1;
    a.cs = ENCODE ? code_store_of(static_cast<const uint8_t *>(out) + a.head) : kStore16;
    a.n_bits = n_bits;
    const size_t per_row = sizeof(float4) + (size_t)a.lut_stride * sizeof(float2);
    // U = 2 (16 KiB of half per block) for tensors that fill the chip with such blocks, else 1; per channel the tables of
    // the rows a chunk overlaps must fit the LDS budget
    int u = a.ng >= (int64_t)kBlock * 2 * 1024 ? 2 : 1;
    auto rows_of = [&](int uu) { return pc ? (int64_t)(kBlock * 16 * uu - 1) / inner + 2 : (int64_t)1; };
    if (pc) {
        if (u == 2 && rows_of(2) * per_row > kCodecLdsBudget) u = 1;
        if (inner < 8 || rows_of(1) * per_row > kCodecLdsBudget) {
            hipLaunchKernelGGL((k_h16_codec_rows<T, ENCODE>), dim3((unsigned)cdiv(C, kBlock)), dim3(kBlock), 0, st, in, out, C,
                               inner, maxval, f, n_bits);
            return launch_rc();
        }
    }
    a.nc_max = (int)rows_of(u);
    a.magic = (pc && inner < kBlock * 16 * u) ? magic_of((int)inner) : 0u;
    const size_t shmem = (size_t)a.nc_max * per_row;
    const dim3 g((unsigned)(a.ng > 0 ? cdiv(a.ng, (int64_t)kBlock * u) : 1));
    if (pc) fp8_launch_u<T, ENCODE, true>(u, g, shmem, st, in, out, maxval, f, a);
    else fp8_launch_u<T, ENCODE, false>(u, g, shmem, st, in, out, maxval, f, a);
    return launch_rc();
}

// argument checks of the two FP8 entry points (everything is reported before any launch); half: the fp16 / bf16 side
int fp8_check(const void *half, const void *codes, int type, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
              float mbits, int n_bits, int sign_bits, QFmt *f)
{
    if (!half_type(type)) return FP8Q_EINVAL;
    if (!half || !codes || !maxval || C <= 0 || inner <= 0 || (n_maxval != 1 && n_maxval != C)) return FP8Q_EINVAL;
    if (n_bits > 8) return FP8Q_EUNSUPPORTED;   // a code is one byte (include/fp8q.h)
    if (int rc = make_fmt(mbits, n_bits, sign_bits, f)) return rc;
    if (n_bits - sign_bits - (int)f->M < 1) return FP8Q_EUNSUPPORTED;   // no exponent bit: 2^(M+1) steps do not fit M bits
    if ((uintptr_t)half & 1) return FP8Q_EINVAL;
    // fp8q_quantize_h16's limits: chunk-local offsets are 32-bit (rows up to 2^30 elements), chunk counts fit gridDim.x
    if ((n_maxval != 1 && inner > (1 << 30)) || C > INT64_MAX / inner || cdiv(C * inner, 16 * kBlock) > (int64_t)INT32_MAX)
        return FP8Q_EINVAL;
    return FP8Q_OK;
}

// ---------------------------------------------------------------------------------------------
// INT codes
// ---------------------------------------------------------------------------------------------
template <class T, int W, bool PC>
__global__ void __launch_bounds__(kBlock)
k_h16_int_encode(const uint16_t *__restrict__ x, void *__restrict__ codes, IntArgs a, int h, int cs)
{
    extern __shared__ float4 kc[];    // nc_max channel constants
    const Chunk c = chunk_setup<PC>(a, kc, ReadRange{a});
    const int tid = threadIdx.x;
    const int len = (int)(c.e1 - c.e0);
    const int ng = len > h ? (len - h) >> 4 : 0;                  // whole groups of this chunk (<= 256): one per lane
    const u4v *xv = reinterpret_cast<const u4v *>(x + c.e0 + h);
    u4v v[2];
    if (tid < ng) {
        v[0] = xv[2 * tid];
        v[1] = xv[2 * tid + 1];
    }

    // the scalars around the groups
    const int64_t s = scalar_of(tid, h, h + 16 * ng, len);
    if (s >= 0 && s < len) {
        const uint32_t q = code_of(T::widen1(x[c.e0 + s]), c.at<PC>((int)s), c.lo, c.hi);
        if (W == 1) static_cast<uint8_t *>(codes)[c.e0 + s] = (uint8_t)q;
        else static_cast<uint16_t *>(codes)[c.e0 + s] = (uint16_t)q;
    }
    if (tid >= ng) return;

    const int off = h + 16 * tid;
    uint32_t q[16];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float e[8];
        widen8<T>(v[k], e);
#pragma unroll
        for (int j = 0; j < 8; ++j) q[8 * k + j] = code_of(e[j], c.at<PC>(off + 8 * k + j), c.lo, c.hi) & (W == 1 ? 0xffu : 0xffffu);
    }
    if (W == 1) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = pack_codes<1>(q + 4 * j);
        store_codes16(static_cast<uint8_t *>(codes) + c.e0 + off, w, cs);
    } else {
        // 2-byte codes: 2 x 16 bytes at whatever 2-byte phase the codes have
        u4v2 *co = reinterpret_cast<u4v2 *>(static_cast<uint16_t *>(codes) + c.e0 + off);
#pragma unroll
        for (int k = 0; k < 2; ++k)
            co[k] = u4v2{pack_codes<2>(q + 8 * k), pack_codes<2>(q + 8 * k + 2), pack_codes<2>(q + 8 * k + 4),
                         pack_codes<2>(q + 8 * k + 6)};
    }
}

template <class T, int W, bool PC>
__global__ void __launch_bounds__(kBlock)
k_h16_int_decode(const void *__restrict__ codes, uint16_t *__restrict__ y, IntArgs a, int h)
{
    extern __shared__ float4 kc[];
    const Chunk c = chunk_setup<PC>(a, kc, ReadRange{a});
    const int tid = threadIdx.x;
    const int len = (int)(c.e1 - c.e0);
    const int ng = len > h ? (len - h) >> 4 : 0;
    // 16 codes: W 16-byte words from the codes' 16-byte boundary on
    const u4v *cv = W == 1 ? reinterpret_cast<const u4v *>(static_cast<const uint8_t *>(codes) + c.e0 + h)
                           : reinterpret_cast<const u4v *>(static_cast<const uint16_t *>(codes) + c.e0 + h);
    u4v v[W];
    if (tid < ng) {
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = cv[W * tid + k];
    }

    const int64_t s = scalar_of(tid, h, h + 16 * ng, len);
    if (s >= 0 && s < len) {
        const uint32_t q = W == 1 ? (uint32_t) static_cast<const uint8_t *>(codes)[c.e0 + s]
                                  : (uint32_t) static_cast<const uint16_t *>(codes)[c.e0 + s];
        y[c.e0 + s] = T::narrow1(value_of<W>(q, c.sgn, c.at<PC>((int)s)));
    }
    if (tid >= ng) return;

    const int off = h + 16 * tid;
    float e[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        constexpr int CPW = 4 / W;     // codes per dword, 4 dwords per 16-byte word
        const u4v vv = v[j / (4 * CPW)];
        const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
        e[j] = value_of<W>(code_at<W>(w[(j / CPW) & 3], j % CPW), c.sgn, c.at<PC>(off + j));
    }
    uint16_t *yo = y + c.e0 + off;
    store_half8<T>(yo, e);
    store_half8<T>(yo + 8, e + 8);
}

template <class T, int W, bool PC>
void int_launch_k(bool encode, const void *in, void *out, const IntArgs &a, hipStream_t st)
{
    const IntPlan p = int_plan(a, false, 2);     // (these kernels have no nontemporal instance either)
    const dim3 g(p.grid_x), b(kBlock);
    const size_t shmem = p.lds_bytes;
    // elements in front of the 16-byte boundary of the side that is loaded 16 bytes at a time (a chunk starts a multiple of
    // 4096 elements behind it, so every chunk has that phase)
    const int lead = (int)((16 - ((uintptr_t)in & 15)) & 15);
    if (encode) {
        const int h = lead >> 1;
        const int cs = W == 1 ? code_store_of(static_cast<const uint8_t *>(out) + h) : kStore16;
        hipLaunchKernelGGL((k_h16_int_encode<T, W, PC>), g, b, shmem, st, static_cast<const uint16_t *>(in), out, a, h, cs);
    } else {
        hipLaunchKernelGGL((k_h16_int_decode<T, W, PC>), g, b, shmem, st, in, static_cast<uint16_t *>(out), a, lead / W);
    }
}

template <class T>
void int_launch_t(bool encode, int W, bool pc, const void *in, void *out, const IntArgs &a, hipStream_t st)
{
    if (W == 1 && pc) int_launch_k<T, 1, true>(encode, in, out, a, st);
    else if (W == 1) int_launch_k<T, 1, false>(encode, in, out, a, st);
    else if (pc) int_launch_k<T, 2, true>(encode, in, out, a, st);
    else int_launch_k<T, 2, false>(encode, in, out, a, st);
}

// argument checks (those of fp8q_int_encode / fp8q_int_decode, and the half side's) and the one launch
int int_codec_launch(bool encode, const void *in, void *out, int type, int64_t C, int64_t inner, const float *delta,
                     const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits, int symmetric,
                     float eps, hipStream_t st)
{
    if (!half_type(type)) return FP8Q_EINVAL;
    if (int rc = int_check_x(in, out, C, inner, n_delta)) return rc;
    IntArgs a = {};
    if (int rc = int_fixed_args(a, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps)) return rc;
    const int W = n_bits <= 8 ? 1 : 2;
    const uintptr_t phalf = (uintptr_t)(encode ? in : out), pcodes = (uintptr_t)(encode ? out : in);
    if ((phalf & 1) || (pcodes & (uintptr_t)(W - 1))) return FP8Q_EINVAL;
    const bool pc = n_delta > 1;
    int_geometry(a, C, inner, pc);
    if (type == FP8Q_DT_F16) int_launch_t<F16>(encode, W, pc, in, out, a, st);
    else int_launch_t<BF16>(encode, W, pc, in, out, a, st);
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_encode_h16(const void *x, uint8_t *codes, int x_type, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                    float mbits, int n_bits, int sign_bits, fp8q_stream_t stream)
{
    QFmt f;
    if (int rc = fp8_check(x, codes, x_type, C, inner, maxval, n_maxval, mbits, n_bits, sign_bits, &f)) return rc;
    const bool pc = n_maxval != 1;
    if (x_type == FP8Q_DT_F16) return fp8_launch<F16, true>(x, codes, C, inner, maxval, pc, f, n_bits, (hipStream_t)stream);
    return fp8_launch<BF16, true>(x, codes, C, inner, maxval, pc, f, n_bits, (hipStream_t)stream);
}

int fp8q_decode_h16(const uint8_t *codes, void *y, int y_type, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                    float mbits, int n_bits, int sign_bits, fp8q_stream_t stream)
{
    QFmt f;
    if (int rc = fp8_check(y, codes, y_type, C, inner, maxval, n_maxval, mbits, n_bits, sign_bits, &f)) return rc;
    const bool pc = n_maxval != 1;
    if (y_type == FP8Q_DT_F16) return fp8_launch<F16, false>(codes, y, C, inner, maxval, pc, f, n_bits, (hipStream_t)stream);
    return fp8_launch<BF16, false>(codes, y, C, inner, maxval, pc, f, n_bits, (hipStream_t)stream);
}

int fp8q_int_encode_h16(const void *x, void *codes, int x_type, int64_t C, int64_t inner, const float *delta,
                        const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits, int symmetric,
                        float eps, fp8q_stream_t stream)
{
    return int_codec_launch(true, x, codes, x_type, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps,
                            (hipStream_t)stream);
}

int fp8q_int_decode_h16(const void *codes, void *y, int y_type, int64_t C, int64_t inner, const float *delta,
                        const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits, int symmetric,
                        float eps, fp8q_stream_t stream)
{
    return int_codec_launch(false, codes, y, y_type, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps,
                            (hipStream_t)stream);
}

}  // extern "C"
