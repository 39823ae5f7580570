// fp8q_rows.h -- what the units of the fp32 quantize / min-max family share (file map: fp8q_quant.hip): the kernel modes,
// the argument blocks of the row-tiled and flat-chunk kernels, the chunk geometry, the launchers called across units.
#pragma once
#include "fp8q_common.h"

namespace {

constexpr int kModeQuant = 0, kModeFused = 1, kModeMinMax = 2;
constexpr int kModeEncode = 3, kModeDecode = 4;   // k_rows_flat only: storage codes (N3) of per-channel short rows

// arguments of k_rows_direct
struct TileArgs {
    int inner;          // row length
    int rows;           // R: rows per tile
    int lut_stride;     // pmax + 1
    int group;          // G: lanes per row (power of two <= 64, or 256 = whole block)
    int coaligned;      // k_rows_direct: x and y share their 16-byte phase -> aligned vector body
    uint32_t magic;     // n / inner      (see magic_of)
    uint32_t lmagic;    // n / lut_stride
};

__device__ __forceinline__ ChanLite lite_lds(const Chan *c)
{
    const float4 h = *reinterpret_cast<const float4 *>(c);   // one ds_read_b128
    ChanLite l;
    l.maxv = h.x;
    l.minv = h.y;
    l.bias = h.z;
    l.pthr = h.w;
    return l;
}

constexpr int kChunkElems = 4096, kChunkGroups = 1024, kFlatMaxCh = 8;
constexpr int kFlatFusedMaxInner = 256;    // fused: rows cut by a chunk border are read by both neighbours; longer
                                           // rows do better in the row-tiled kernel (measured at 576: 4.65 vs 4.32 TB/s)

struct FlatArgs {
    int inner;        // row length (>= 4)
    int rpc;          // table rows per chunk: most rows a window of 4096 (+3 tail) elements can overlap
    int nch;          // chunks per tile (<= kFlatMaxCh)
    int lut_stride;   // pmax + 1
    int group;        // pass A: lanes per row (power of two <= 64); k_rows_staged: log2 of it
    int tail;         // n - 4 * nvec: scalars after the last 16-byte group
    uint32_t magic;   // o / inner
    uint32_t rmagic;  // lr / rpc
    int64_t nvec;     // 16-byte groups in the tensor (>= 1)
    int64_t nchunks;  // ceil(nvec / 1024)
    int n_bits;       // encode / decode: position of the sign bit
    int pad0;
};

struct __attribute__((aligned(16))) ChunkInfo {
    int64_t row_lo;   // first row overlapping the chunk
    int phase;        // offset of the chunk's first element within that row
    int nrows;        // rows overlapping the chunk (tail scalars included)
    int len;          // elements in the chunk's aligned body (multiple of 4, <= 4096)
    int tail;         // scalars after the body (last chunk of the tensor only)
    int pad[2];
};

// elo / inner for 0 <= elo < 2^52, 1 <= inner < 2^31 without the ~200-instruction software 64-bit division: the double
// quotient is within 1 of the integer one; an exact integer remainder fixes it up
__device__ __forceinline__ int64_t div_rows(int64_t elo, int inner)
{
    int64_t q = (int64_t)((double)elo / (double)inner);
    int64_t r = elo - q * inner;
    if (r < 0) --q, r += inner;
    if (r >= inner) ++q;
    return q;
}

// what a short-row launcher returns when the problem does not fit its kernel: the caller takes the next route
constexpr int kNotFlat = -1000;
static_assert(kNotFlat == FP8Q_CODEC_NOT_FLAT, "fp8q_codec_flat_launch passes the code through");

// table rows per chunk: most rows a window of 4096 (+3 tail) elements can overlap
inline int64_t flat_rpc(int64_t inner) { return (inner + (kChunkElems + 3) - 2) / inner + 1; }

// LDS per table row of the flat-chunk kernels: head patch (16 B) + channel constants (16 B) + pmax + 1 entries {s, 1/s}
// (+ the row's maxval when the kernel finds it itself)
inline int64_t flat_per_row(int lut_stride, bool fused = false) { return 16 + 16 + (int64_t)lut_stride * 8 + (fused ? 4 : 0); }

// The chunk geometry of [C, inner] (inner >= 4) cut into aligned 4096-element chunks; nch and group are the launcher's.
inline FlatArgs flat_geometry(int64_t C, int64_t inner, int lut_stride)
{
    FlatArgs a = {};
    a.inner = (int)inner;
    a.lut_stride = lut_stride;
    a.magic = magic_of((int)inner);
    const int64_t n = C * inner;
    a.nvec = n >> 2;
    a.tail = (int)(n & 3);
    a.nchunks = cdiv(a.nvec, kChunkGroups);
    a.rpc = (int)flat_rpc(inner);
    a.rmagic = magic_of(a.rpc);
    return a;
}

// The one launch site of a row launcher: route_emit (fp8q_common.h) on the row family's record.
template <class Fill, class Launch>
inline int rows_emit(fp8q_rows_route_info *rec, Fill &&fill, Launch &&launch)
{
    return route_emit(rec, fill, launch);
}

}  // namespace

// The short-row launchers called from other units of the library: hidden, not part of the C ABI.  (C linkage because
// FoldArgs has internal linkage -- every unit has its own copy of fp8q_common.h -- which a C++ signature would inherit.)
// Each returns kNotFlat when the shape does not suit its kernel.  rec: record the route instead of launching (rows_emit).
#define FP8Q_HIDDEN extern "C" __attribute__((visibility("hidden")))
FP8Q_HIDDEN int64_t fp8q_direct_max_inner();
FP8Q_HIDDEN int fp8q_launch_rows_direct(int mode, const float *x, float *y, int64_t C, int64_t inner, const float *maxval,
                                   float *row_min, float *row_max, float *maxval_out, const QFmt &f, const FoldArgs &fa,
                                   hipStream_t st, fp8q_rows_route_info *rec);
FP8Q_HIDDEN int fp8q_launch_rows_reg(bool quant, const float *x, float *y, int64_t C, int64_t inner, float *row_min, float *row_max,
                                float *maxval_out, const QFmt &f, const FoldArgs &fa, hipStream_t st, fp8q_rows_route_info *rec);
FP8Q_HIDDEN int fp8q_launch_rows_staged_mm(const float *x, int64_t C, int64_t inner, float *row_min, float *row_max,
                                      float *maxval_out, const FoldArgs &fa, hipStream_t st, fp8q_rows_route_info *rec);
// The three entries behind their argument checks (fp8q_quantize_f32, fp8q_minmax_quantize_f32, fp8q_minmax_f32 and its
// packed / linspace variants): what fp8q_rows_route runs with rec set.
FP8Q_HIDDEN int fp8q_quantize_plan(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                              float mbits, int n_bits, int sign_bits, hipStream_t st, fp8q_rows_route_info *rec);
FP8Q_HIDDEN int fp8q_minmax_quantize_plan(const float *x, float *y, int64_t C, int64_t inner, float *row_min, float *row_max,
                                     float *maxval_out, float mbits, int n_bits, int sign_bits, hipStream_t st,
                                     fp8q_rows_route_info *rec);
FP8Q_HIDDEN int fp8q_minmax_plan(const float *x, int64_t C, int64_t inner, fp8q_rows_route_info *rec);
