// fp8q_quant.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the quantize / min-max family + their C ABI
// (include/fp8q.h).  The family is five of the library's sixteen translation units: this one (long rows, formats chosen on
// the device), fp8q_rows.hip + fp8q_rowsreg.hip (short per-channel rows), fp8q_minmax.hip and fp8q_multi.hip; fp8q_rows.h
// holds what they share, fp8q_common.h what every unit shares, fp8q_device.h the per-element arithmetic.
//
// Every kernel here is elementwise or a reduction: the roofline is HBM bandwidth, not MFMA.
// Common shape: 256-thread blocks (4 waves, one per SIMD), 16 B per lane per memory instruction
// (1 KiB per wave-instruction), 4 independent loads in flight per lane, and -- what HBM turned out to
// care about most (a copy-kernel sweep: docs/HISTORY.md) -- every block moves ALIGNED 16 KiB pieces, neighbouring
// blocks neighbouring pieces, one piece (or one short tile) per block rather than a persistent grid.
//
// Kernels of the family:
//   k_quant_rows      K1, one channel per blockIdx.y (per-tensor: one row).  Scale LUT in LDS.            fp8q_quant.hip
//   k_quant_scalar    K1 fallback for x / y that are not 16-byte co-aligned.                               fp8q_quant.hip
//   k_copy            float4 copy with K1's launch geometry (measured HBM ceiling).                        fp8q_quant.hip
//   k_rows_flat       per-channel tensors with short rows, cut into aligned 4096-element chunks regardless of
//                     the rows (per-row tables in LDS): MODE 0 = K1, MODE 1 = K2+K5+K1 fused (rows <= 256). fp8q_rows.hip
//   k_rows_staged     K2+K5+K1 fused for rows <= 256 elements of any length (147): the aligned chunk is fetched once and
//                     parked in LDS; k_rows_staged_mm = its K2 (+fold) twin for rows of 4..256 elements.   fp8q_rows.hip
//   k_rows_direct     round-1 row-tiled kernel: rows too short for per-row tables, unaligned pointers, the
//                     fused / K2 cases the kernels above do not take.                                      fp8q_rows.hip
//   k_rows_reg        K2+K5+K1 fused, or K2 alone, for rows of 128..8192 elements: the row in registers.  fp8q_rowsreg.hip
//   k_multi_flat      multi-tensor K1: one block = one chunk of one of <= 32 tensors.                      fp8q_multi.hip
//   k_minmax_partial  K2/K3 stage 1: per-(row, split) min / max / NaN flag  (stage 2 + K5: fp8q_common.h). fp8q_minmax.hip
#include "fp8q_rows.h"
#include "fp8q_select.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K1 rows: blockIdx.y = row (channel), blockIdx.x strides over the row.  {s, 1/s} table in LDS.
// ---------------------------------------------------------------------------------------------
// U = 16-byte groups per lane and step: 4 (16 KiB pieces per block), or 1 for cache-sized tensors, whose launches are
// latency-bound and want four times the blocks (as k_affine_act: fp8q_epilogue.hip)
template <bool NT, int U>
__device__ __forceinline__ void quant_rows_body(const float *__restrict__ x, float *__restrict__ y, int64_t inner,
                                                const float *__restrict__ maxval, int per_channel, const QFmt &f)
{
    __shared__ float2 lut[kLutMax];
    const int row = blockIdx.y;
    const int tid = threadIdx.x;
    const Chan cfull = make_chan(maxval[per_channel ? row : 0], f);
    for (int i = tid; i <= f.pmax; i += kBlock) lut[i] = lut_entry(cfull, i, f.M);
    __syncthreads();
    const ChanLite c = lite(cfull);
    const float pmaxf = (float)f.pmax;
    const float qthr = f.qthr;

    const float *xr = x + (int64_t)row * inner;
    float *yr = y + (int64_t)row * inner;
    // peel to 16-byte alignment (x and y are co-aligned: checked on the host)
    int64_t head = ((16 - ((uintptr_t)xr & 15)) & 15) >> 2;
    if (head > inner) head = inner;
    const int64_t nvec = (inner - head) >> 2;
    const int64_t tail0 = head + (nvec << 2);
    if (blockIdx.x == 0) {
        if (tid < head) yr[tid] = quant_one(xr[tid], c, lut, pmaxf, qthr);
        const int64_t t = tail0 + tid;
        if (t < inner) yr[t] = quant_one(xr[t], c, lut, pmaxf, qthr);
    }
    const vf4 *xv = reinterpret_cast<const vf4 *>(xr + head);
    vf4 *yv = reinterpret_cast<vf4 *>(yr + head);

    const int64_t step = (int64_t)gridDim.x * (kBlock * U);
    for (int64_t base = (int64_t)blockIdx.x * (kBlock * U); base < nvec; base += step) {
        if (base + kBlock * U <= nvec) {
            vf4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = ld16<NT>(xv + base + u * kBlock + tid);
            float e[U * 4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                e[4 * u + 0] = v[u].x;
                e[4 * u + 1] = v[u].y;
                e[4 * u + 2] = v[u].z;
                e[4 * u + 3] = v[u].w;
            }
            quant_group<U * 4>(e, c, lut, pmaxf, qthr);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                vf4 w = {e[4 * u + 0], e[4 * u + 1], e[4 * u + 2], e[4 * u + 3]};
                st16<NT>(yv + base + u * kBlock + tid, w);
            }
        } else {
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + u * kBlock + tid;
                if (i < nvec) {
                    const vf4 w = ld16<NT>(xv + i);
                    float e[4] = {w.x, w.y, w.z, w.w};
                    quant_group<4>(e, c, lut, pmaxf, qthr);
                    vf4 o = {e[0], e[1], e[2], e[3]};
                    st16<NT>(yv + i, o);
                }
            }
        }
    }
}

template <bool NT, int U>
__global__ void __launch_bounds__(kBlock)
k_quant_rows(const float *__restrict__ x, float *__restrict__ y, int64_t inner,
             const float *__restrict__ maxval, int per_channel, QFmt f)
{
    quant_rows_body<NT, U>(x, y, inner, maxval, per_channel, f);
}

// K1 scalar fallback (x / y not 16-byte co-aligned): one row per blockIdx.y, dword accesses
__device__ __forceinline__ void quant_scalar_body(const float *__restrict__ x, float *__restrict__ y, int64_t inner,
                                                  const float *__restrict__ maxval, int per_channel, const QFmt &f)
{
    __shared__ float2 lut[kLutMax];
    const int row = blockIdx.y;
    const Chan cfull = make_chan(maxval[per_channel ? row : 0], f);
    for (int i = threadIdx.x; i <= f.pmax; i += kBlock) lut[i] = lut_entry(cfull, i, f.M);
    __syncthreads();
    const ChanLite c = lite(cfull);
    const float *xr = x + (int64_t)row * inner;
    float *yr = y + (int64_t)row * inner;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < inner;
         i += (int64_t)gridDim.x * kBlock)
        yr[i] = quant_one(xr[i], c, lut, (float)f.pmax, f.qthr);
}

__global__ void __launch_bounds__(kBlock)
k_quant_scalar(const float *__restrict__ x, float *__restrict__ y, int64_t inner,
               const float *__restrict__ maxval, int per_channel, QFmt f)
{
    quant_scalar_body(x, y, inner, maxval, per_channel, f);
}

// K1 with the mantissa width read from DEVICE memory (fp8q_quantize_dm_f32): the MSE estimator's plurality vote on the
// mantissa bits (range_estimators.py:350-354) stays on the GPU, and the batch that follows it in the same calibration
// forward is quantized with the winner without a host round trip.  The host cannot know the format, so it passes the
// constants of every width the call admits (M = 1 .. n_bits - sign_bits); calibration-only path: one row per
// blockIdx.y whatever the row length (the by-value kernels keep their tuned routes).
struct FmtSel {
    const float *mbits_dev;
    const unsigned char *signed_dev;   // fp8q_quantize_ds_f32: the SIGN in device memory instead (1: tab[0], 0: tab[1]), else null
    int hi;           // n_bits - sign_bits
    QFmt tab[8];      // tab[M - 1]
};

__device__ __forceinline__ QFmt pick_fmt(const FmtSel &s)
{
    if (s.signed_dev) return s.tab[*s.signed_dev ? 0 : 1];
    float M = rintf(*s.mbits_dev);                       // torch.round: half to even (fp8_quantizer.py:105)
    M = fminf(fmaxf(M, 1.0f), (float)s.hi);              // NaN -> 1 (the by-value entry point refuses NaN on the host)
    return s.tab[(int)M - 1];
}

// width AND sign in device memory (fp8q_quantize_dms_f32: an MSE estimator's vote next to the flag of fp8q_sign_fold_u8)
struct FmtSel2 {
    const float *mbits_dev;
    const unsigned char *signed_dev;
    int hi[2];          // n_bits - sign_bits for sign_bits = 1, 0
    QFmt tab[2][8];     // tab[1 - sign_bits][M - 1]
};

__device__ __forceinline__ QFmt pick_fmt(const FmtSel2 &s)
{
    const int u = *s.signed_dev ? 0 : 1;
    float M = rintf(*s.mbits_dev);
    M = fminf(fmaxf(M, 1.0f), (float)s.hi[u]);
    return s.tab[u][(int)M - 1];
}

template <bool NT, int U, class SEL>
__global__ void __launch_bounds__(kBlock)
k_quant_rows_dm(const float *__restrict__ x, float *__restrict__ y, int64_t inner, const float *__restrict__ maxval,
                int per_channel, SEL sel)
{
    const QFmt f = pick_fmt(sel);
    quant_rows_body<NT, U>(x, y, inner, maxval, per_channel, f);
}

// K1 of a per-tensor quantizer whose winner -- mantissa width and clipping value -- is still the MSE table of the search that ran
// just before it (fp8q_mse_calibrate_f32 with the mantissa search): every workgroup takes the selection for itself -- a few
// loads per thread from L2 (n_m x n_cand <= 8 x 128 entries), the reference's two-level vote (range_estimators.py:350-369 with
// one channel) as ONE arg-min over the table in (width, candidate) order: the smallest entry, the first of equals, a NaN before
// everything -- and workgroup 0 writes the estimator's outputs.  The kernel boundary makes the table visible: no tickets, no
// agent-scope traffic in the launch that finishes the table (k_mse_eval with the selection appended: 20.4 us per MobileNetV2
// activation with six widths, 12.5 without).
struct SelIn {
    const float *mses, *grid;
    int n_m, n_cand;
    SelOne so;
};

template <bool NT, int U>
__global__ void __launch_bounds__(kBlock)
k_quant_rows_sel(const float *__restrict__ x, float *__restrict__ y, int64_t inner, FmtSel sel, SelIn si)
{
    __shared__ float s_v[kBlock / 64], s_g[kBlock / 64];
    __shared__ int s_i[kBlock / 64];
    __shared__ float s_mv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = si.n_m * si.n_cand;
    ArgMin a = {__builtin_inff(), 0x7fffffff};
    float ag = 0.0f;
    for (int i0 = 0; i0 < total; i0 += 4 * kBlock) {
        float t[4], g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                 // (all loads of a trip before the first use)
            const int i = i0 + q * kBlock + tid;
            t[q] = i < total ? si.mses[i] : 0.0f;
            g[q] = i < total ? si.grid[i % si.n_cand] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * kBlock + tid;
            const ArgMin o = {t[q], i};
            if (i < total && argmin_less(o, a)) {
                a = o;
                ag = g[q];
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ArgMin o;
        o.v = __shfl_xor(a.v, off, 64);
        o.idx = __shfl_xor(a.idx, off, 64);
        const float og = __shfl_xor(ag, off, 64);
        if (argmin_less(o, a)) {
            a = o;
            ag = og;
        }
    }
    if (lane == 0) {
        s_v[wave] = a.v;
        s_i[wave] = a.idx;
        s_g[wave] = ag;
    }
    __syncthreads();
    a = ArgMin{s_v[0], s_i[0]};
    ag = s_g[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) {
        const ArgMin o = {s_v[w], s_i[w]};
        if (argmin_less(o, a)) {
            a = o;
            ag = s_g[w];
        }
    }
    const int vote = a.idx / si.n_cand;
    const float mb = si.so.M[vote];
    if (tid == 0) {
        s_mv = ag;
        if (blockIdx.x == 0 && blockIdx.y == 0) {
            si.so.mbits_out[0] = mb;
            if (si.so.vote_out) si.so.vote_out[0] = vote;
            si.so.maxval_out[0] = ag;
            if (si.so.xmin_out) si.so.xmin_out[0] = si.so.sign * ag;      // sign_bits * -1.0 * maxval (:369)
        }
    }
    __syncthreads();
    float M = rintf(mb);
    M = fminf(fmaxf(M, 1.0f), (float)sel.hi);
    const QFmt f = sel.tab[(int)M - 1];
    quant_rows_body<NT, U>(x, y, inner, &s_mv, 0, f);
}

// Short per-channel rows with the width in device memory (MobileNetV2's weights in the mantissa search: [1280, 320],
// [96, 1, 3, 3] ...): a WAVE per row -- its channel constants and {s, 1/s} table built once per wave in the wave's own slice of
// LDS, the row streamed by its 64 lanes -- instead of a 256-thread workgroup (and a ~50-operation double-precision set-up) per
// row of a few hundred elements.  Same arithmetic as quant_rows_body (quant_one), bit for bit.
template <class SEL>
__global__ void __launch_bounds__(kBlock)
k_quant_short_rows_dm(const float *__restrict__ x, float *__restrict__ y, int64_t C, int inner, const float *__restrict__ maxval,
                      SEL sel)
{
    __shared__ float2 lut[kBlock / 64][kLutMax];
    const QFmt f = pick_fmt(sel);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float pmaxf = (float)f.pmax;
    for (int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + wave; row < C; row += (int64_t)gridDim.x * (kBlock / 64)) {
        const Chan cfull = make_chan(maxval[row], f);
        for (int i = lane; i <= f.pmax; i += 64) lut[wave][i] = lut_entry(cfull, i, f.M);
        __builtin_amdgcn_wave_barrier();
        const ChanLite c = lite(cfull);
        const float *xr = x + row * inner;
        float *yr = y + row * inner;
        for (int i = lane; i < inner; i += 64) yr[i] = quant_one(xr[i], c, lut[wave], pmaxf, f.qthr);
        __builtin_amdgcn_wave_barrier();       // (the next row's table overwrites this one)
    }
}

template <class SEL>
__global__ void __launch_bounds__(kBlock)
k_quant_scalar_dm(const float *__restrict__ x, float *__restrict__ y, int64_t inner, const float *__restrict__ maxval,
                  int per_channel, SEL sel)
{
    const QFmt f = pick_fmt(sel);
    quant_scalar_body(x, y, inner, maxval, per_channel, f);
}

// 16-byte-per-lane copy with K1's launch shape: the achievable-HBM yardstick
template <bool NT>
__global__ void __launch_bounds__(kBlock)
k_copy(const vf4 *__restrict__ x, vf4 *__restrict__ y, int64_t nvec)
{
    const int tid = threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * (kBlock * kUnroll);
    for (int64_t base = (int64_t)blockIdx.x * (kBlock * kUnroll); base < nvec; base += step) {
        if (base + kBlock * kUnroll <= nvec) {
            vf4 v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) v[u] = ld16<NT>(x + base + u * kBlock + tid);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) st16<NT>(y + base + u * kBlock + tid, v[u]);
        } else {
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t i = base + u * kBlock + tid;
                if (i < nvec) st16<NT>(y + i, ld16<NT>(x + i));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The launch shape of the long-row kernels for C rows of `inner` elements (C <= 65535: gridDim.y).
// One 16 KiB piece per block for big tensors (measured: 6.3 TB/s against 5.8 with a persistent grid of 2048
// blocks at 1 GiB; small tensors prefer the smaller grid); a partial last piece of a row gets no block of its own
// (k_copy's rule counts it: partial_piece).  Per-tensor rows below small_elems run 4 KiB pieces (U = 1): their launches
// are latency-bound and want four times the blocks; a per-channel block also builds its row's table, so never there.
// total_cap(nt, pieces of the whole tensor) is the caller's block cap.
// ---------------------------------------------------------------------------------------------
struct RowGrid {
    bool nt;       // nontemporal: the tensor is beyond the caches
    bool small;    // cache-sized per-tensor row
    int64_t bx;    // blocks per row of the 16-byte kernels
    int64_t bs;    // blocks per row of the scalar fallback
};

constexpr int64_t kSmallElems = (int64_t)8 << 20;   // FP8Q_K1_SMALL_M (fp8q_quantize_f32 only)

// cache-sized tensors (< 64 MiB): a resident grid of 2048 blocks with the same number of pieces each, not several
// ragged rounds of one-piece blocks ([64,128,28,28] 12.2 -> 10.9 us, [64,144,28,28] 13.0 -> 11.6, [64,24,56,56]
// 10.0 -> 9.0 by rocprofv3); tensors beyond the caches: one piece per block
inline int64_t k1_total_cap(bool nt, int64_t pieces, int64_t big_cap = 65536)
{
    return (!nt || pieces <= 4096) ? kTargetBlocks : big_cap;
}

template <class CapRule>
RowGrid row_grid(int64_t C, int64_t inner, int64_t small_elems, CapRule total_cap, bool partial_piece = false)
{
    RowGrid g;
    g.nt = C * inner * 4 >= kNtBytes;
    g.small = C == 1 && inner < small_elems;
    const int64_t per = 4 * kBlock * (g.small ? 1 : kUnroll);
    const int64_t pieces = partial_piece ? cdiv(inner, per) : (inner / per > 0 ? inner / per : 1);
    const int64_t total = total_cap(g.nt, pieces * C);
    const int64_t cap = total / C > 0 ? total / C : 1;
    g.bx = balanced_blocks(pieces, cap);
    g.bs = cdiv(inner, kBlock) < cap * 4 ? cdiv(inner, kBlock) : cap * 4;
    return g;
}

// the three instantiations every K1 family has: f(NT, U) with nontemporal 16 KiB pieces, cached 4 KiB pieces, cached 16 KiB
template <class F>
void dispatch_k1(const RowGrid &g, F &&f)
{
    if (g.nt) f(Const<true>{}, Const<kUnroll>{});
    else if (g.small) f(Const<false>{}, Const<1>{});
    else f(Const<false>{}, Const<kUnroll>{});
}

// the constants of every mantissa width a device-selected format may take: tab[M - 1], widths above hi repeat hi's
int fill_widths(QFmt tab[8], int hi, int n_bits, int sign_bits)
{
    if (hi < 1 || hi > 8) return FP8Q_EINVAL;
    for (int M = 1; M <= 8; ++M)
        if (int rc = make_fmt((float)(M <= hi ? M : hi), n_bits, sign_bits, &tab[M - 1])) return rc;
    return FP8Q_OK;
}

}  // namespace

extern "C" {

int fp8q_version(void) { return FP8Q_VERSION; }

const char *fp8q_strerror(int code)
{
    switch (code) {
        case FP8Q_OK: return "ok";
        case FP8Q_EINVAL: return "invalid argument";
        case FP8Q_EUNSUPPORTED: return "unsupported format (more than 7 exponent bits)";
        case FP8Q_EWORKSPACE: return "workspace too small or misaligned";
        case FP8Q_ETOOLONG: return "rows longer than fp8q_fused_max_inner(): use fp8q_minmax_f32 + fp8q_quantize_f32";
        case FP8Q_ETOOMANY: return "more than 65535 channels in one MSE grid-search call";
        case FP8Q_ETIMEDOUT: return "a min/max reducer block timed out waiting for its streaming blocks (that call's range is NaN)";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

int fp8q_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval,
                      int64_t n_maxval, float mbits, int n_bits, int sign_bits, fp8q_stream_t stream)
{
    return fp8q_quantize_plan(x, y, C, inner, maxval, n_maxval, mbits, n_bits, sign_bits, (hipStream_t)stream, nullptr);
}

// fp8q_quantize_f32 itself; rec: record the route instead of launching (rows_emit, fp8q_rows.h)
int fp8q_quantize_plan(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                       float mbits, int n_bits, int sign_bits, hipStream_t st, fp8q_rows_route_info *rec)
{
    if (C < 0 || inner < 0 || (n_maxval != 1 && n_maxval != C)) return FP8Q_EINVAL;
    QFmt f;
    if (int rc = make_fmt(mbits, n_bits, sign_bits, &f)) return rc;
    if (C == 0 || inner == 0) return FP8Q_OK;   // empty tensor: nothing to do (pointers may be null)
    if (!x || !y || !maxval) return FP8Q_EINVAL;
    const int per_channel = n_maxval != 1;
    if (!per_channel) {  // one row
        inner *= C;
        C = 1;
    }
    const bool aligned = (((uintptr_t)x ^ (uintptr_t)y) & 15) == 0 && ((uintptr_t)x & 3) == 0;

    if (per_channel && inner <= fp8q_direct_max_inner() && ((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0) {
        // short rows: G lanes per row, tables in LDS
        const FoldArgs nofold = {0, 1, 0.0f, 0.0f};
        return fp8q_launch_rows_direct(kModeQuant, x, y, C, inner, maxval, nullptr, nullptr, nullptr, f, nofold, st, rec);
    }
    if (C > 65535) {
        // very many long rows: one launch per 65535 rows (gridDim.y limit)
        for (int64_t c0 = 0; c0 < C; c0 += 65535) {
            const int64_t cn = (C - c0) < 65535 ? (C - c0) : 65535;
            int rc = fp8q_quantize_plan(x + c0 * inner, y + c0 * inner, cn, inner, maxval + c0, cn,
                                        mbits, n_bits, sign_bits, st, rec);
            if (rc) return rc;
        }
        return FP8Q_OK;
    }
    static const int k1_blocks_env = env_int("FP8Q_K1_BLOCKS", 0, 0);   // tuning knob: total block cap
    static const int64_t small_elems = [] {   // FP8Q_K1_SMALL_M: tensors below this many Mi elements run 4 KiB pieces per block
        const char *e = getenv("FP8Q_K1_SMALL_M");
        const long v = e ? atol(e) : -1;
        return v >= 0 ? (int64_t)v << 20 : kSmallElems;
    }();
    const RowGrid g = row_grid(C, inner, small_elems, [](bool nt, int64_t pieces) {
        return k1_blocks_env > 0 ? (int64_t)k1_blocks_env : k1_total_cap(nt, pieces);
    });
    const auto fill = [&](fp8q_rows_route_info &r) {
        r.kernel = aligned ? FP8Q_ROWS_K_QUANT_ROWS : FP8Q_ROWS_K_QUANT_SCALAR;
        r.nontemporal = aligned && g.nt;      // (the scalar fallback has one instance)
        r.small = aligned && !g.nt && g.small;
        r.grid_x = aligned ? g.bx : g.bs;
        r.grid_y = C;
    };
    return rows_emit(rec, fill, [&] {
        if (aligned) {
            dispatch_k1(g, [&](auto NT, auto U) {
                hipLaunchKernelGGL((k_quant_rows<NT(), U()>), dim3((unsigned)g.bx, (unsigned)C), dim3(kBlock), 0, st, x, y, inner,
                                   maxval, per_channel, f);
            });
        } else {
            hipLaunchKernelGGL(k_quant_scalar, dim3((unsigned)g.bs, (unsigned)C), dim3(kBlock), 0, st, x, y, inner, maxval, per_channel, f);
        }
    });
}

// Which kernel of the row family a call of the three entries reaches: the entries' own code behind their argument checks
// (fp8q_quantize_plan, fp8q_minmax_quantize_plan, fp8q_minmax_plan) run with a record instead of a stream, on made-up
// addresses that have the caller's 16-byte phases and are never dereferenced.  Host arithmetic only.
int fp8q_rows_route(int op, int64_t C, int64_t inner, int per_channel, float mbits, int n_bits, int sign_bits, int x_mod16,
                    int y_mod16, int in_place, fp8q_rows_route_info *info)
{
    if (!info || op < FP8Q_ROWS_QUANTIZE || op > FP8Q_ROWS_MINMAX_QUANTIZE || C < 0 || inner < 0) return FP8Q_EINVAL;
    if (x_mod16 < 0 || x_mod16 > 15 || y_mod16 < 0 || y_mod16 > 15) return FP8Q_EINVAL;
    if (in_place && op != FP8Q_ROWS_MINMAX && y_mod16 != x_mod16) return FP8Q_EINVAL;
    // far apart, far from null, and far from wrapping at any tensor the entries take
    const float *x = reinterpret_cast<const float *>(((uintptr_t)1 << 44) + (uintptr_t)x_mod16);
    float *y = in_place ? const_cast<float *>(x) : reinterpret_cast<float *>(((uintptr_t)1 << 45) + (uintptr_t)y_mod16);
    float *rng = reinterpret_cast<float *>((uintptr_t)1 << 46);
    fp8q_rows_route_info r = {};
    r.kernel = -1;      // an empty tensor: nothing is launched
    int rc;
    if (op == FP8Q_ROWS_QUANTIZE) {
        rc = fp8q_quantize_plan(x, y, C, inner, rng, per_channel ? C : 1, mbits, n_bits, sign_bits, nullptr, &r);
    } else if (op == FP8Q_ROWS_MINMAX_QUANTIZE) {
        rc = fp8q_minmax_quantize_plan(x, y, C, inner, rng, rng, rng, mbits, n_bits, sign_bits, nullptr, &r);
    } else {
        if (!per_channel) {   // the wrapper's view of a per-tensor estimator: one row
            inner *= C;
            C = C > 0 ? 1 : 0;
        }
        rc = fp8q_minmax_plan(x, C, inner, &r);
    }
    if (rc == FP8Q_OK) *info = r;
    return rc;
}

}  // extern "C"

// the launch geometry shared by the entry points whose format is chosen on the device (width: fp8q_quantize_dm_f32, sign:
// fp8q_quantize_ds_f32)
template <class SEL>
static int quantize_sel_launch(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                               const SEL &sel, fp8q_stream_t stream)
{
    if (C == 0 || inner == 0) return FP8Q_OK;
    if (!x || !y || !maxval) return FP8Q_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int per_channel = n_maxval != 1;
    if (!per_channel) {
        inner *= C;
        C = 1;
    }
    if (per_channel && inner <= 2048 && inner < (1ll << 31) / 4) {
        // short rows: a wave per row
        const int64_t blocks = cdiv(C, kBlock / 64);
        hipLaunchKernelGGL(k_quant_short_rows_dm<SEL>, dim3((unsigned)(blocks < 8 * kTargetBlocks ? blocks : 8 * kTargetBlocks)), dim3(kBlock), 0, st,
                           x, y, C, (int)inner, maxval, sel);
        return launch_rc();
    }
    for (int64_t c0 = 0; c0 < C; c0 += 65535) {   // gridDim.y limit
        const int64_t cn = (C - c0) < 65535 ? (C - c0) : 65535;
        const float *xs = x + c0 * inner;
        float *ys = y + c0 * inner;
        const float *mvp = maxval + (per_channel ? c0 : 0);
        // k_quant_rows peels every row to 16-byte alignment assuming x and y rows are co-aligned
        const bool aligned = (((uintptr_t)xs ^ (uintptr_t)ys) & 15) == 0 && ((uintptr_t)xs & 3) == 0;
        // the geometry of fp8q_quantize_f32 (nontemporal beyond the caches, 4 KiB pieces on a resident grid for cache-sized
        // per-tensor rows): the format is the only thing this entry point does not know on the host
        const RowGrid g = row_grid(cn, inner, kSmallElems, [](bool nt, int64_t pieces) { return k1_total_cap(nt, pieces); });
        if (aligned) {
            dispatch_k1(g, [&](auto NT, auto U) {
                hipLaunchKernelGGL((k_quant_rows_dm<NT(), U(), SEL>), dim3((unsigned)g.bx, (unsigned)cn), dim3(kBlock), 0, st, xs, ys,
                                   inner, mvp, per_channel, sel);
            });
        } else {
            hipLaunchKernelGGL(k_quant_scalar_dm<SEL>, dim3((unsigned)g.bs, (unsigned)cn), dim3(kBlock), 0, st, xs, ys, inner,
                               mvp, per_channel, sel);
        }
        if (int rc = launch_rc()) return rc;
    }
    return FP8Q_OK;
}

extern "C" {

int fp8q_quantize_dm_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                         const float *mbits_dev, int n_bits, int sign_bits, fp8q_stream_t stream)
{
    if (C < 0 || inner < 0 || (n_maxval != 1 && n_maxval != C) || !mbits_dev) return FP8Q_EINVAL;
    FmtSel sel;
    sel.mbits_dev = mbits_dev;
    sel.signed_dev = nullptr;
    sel.hi = n_bits - sign_bits;
    if (int rc = fill_widths(sel.tab, sel.hi, n_bits, sign_bits)) return rc;
    return quantize_sel_launch(x, y, C, inner, maxval, n_maxval, sel, stream);
}

// K1 of a quantizer with allow_unsigned whose sign_bits is still a flag in device memory (fp8q_sign_fold_u8): both formats
// of the width travel by value, the kernel reads the flag (fp8_quantizer.py:216-225 decides it with a host round trip).
int fp8q_quantize_ds_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                         float mbits, int n_bits, const unsigned char *signed_flag, fp8q_stream_t stream)
{
    if (C < 0 || inner < 0 || (n_maxval != 1 && n_maxval != C) || !signed_flag) return FP8Q_EINVAL;
    FmtSel sel;
    sel.mbits_dev = nullptr;
    sel.signed_dev = signed_flag;
    sel.hi = 2;
    if (int rc = make_fmt(mbits, n_bits, 1, &sel.tab[0])) return rc;
    if (int rc = make_fmt(mbits, n_bits, 0, &sel.tab[1])) return rc;
    for (int i = 2; i < 8; ++i) sel.tab[i] = sel.tab[1];
    return quantize_sel_launch(x, y, C, inner, maxval, n_maxval, sel, stream);
}

// ... and with the mantissa width in device memory as well (the MSE estimator's vote for a quantizer whose sign is still
// pending): 2 x 8 formats by value.
int fp8q_quantize_dms_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                          const float *mbits_dev, int n_bits, const unsigned char *signed_flag, fp8q_stream_t stream)
{
    if (C < 0 || inner < 0 || (n_maxval != 1 && n_maxval != C) || !mbits_dev || !signed_flag) return FP8Q_EINVAL;
    FmtSel2 sel;
    sel.mbits_dev = mbits_dev;
    sel.signed_dev = signed_flag;
    for (int u = 0; u < 2; ++u) {
        sel.hi[u] = n_bits - (1 - u);
        if (int rc = fill_widths(sel.tab[u], sel.hi[u], n_bits, 1 - u)) return rc;
    }
    return quantize_sel_launch(x, y, C, inner, maxval, n_maxval, sel, stream);
}

}  // extern "C"

// (called from fp8q_mse.hip: the last step of fp8q_mse_calibrate_f32 for a per-tensor quantizer with the mantissa search)
// Returns FP8Q_EUNSUPPORTED when the tensor does not take the aligned vector kernel: the caller then selects in its own launch.
int fp8q_quantize_select_f32(const float *x, float *y, int64_t n, const float *mses, const float *grid, int n_m, int n_cand,
                             const SelOne *so, int n_bits, int sign_bits, hipStream_t st)
{
    FmtSel sel;
    sel.mbits_dev = nullptr;
    sel.signed_dev = nullptr;
    sel.hi = n_bits - sign_bits;
    if (n_m < 1 || n_m > kSelMaxM || n_cand < 1 || !so || !x || !y || n <= 0) return FP8Q_EINVAL;
    if (int rc = fill_widths(sel.tab, sel.hi, n_bits, sign_bits)) return rc;
    const bool aligned = (((uintptr_t)x ^ (uintptr_t)y) & 15) == 0 && ((uintptr_t)x & 3) == 0;
    if (!aligned) return FP8Q_EUNSUPPORTED;
    SelIn si;
    si.mses = mses;
    si.grid = grid;
    si.n_m = n_m;
    si.n_cand = n_cand;
    si.so = *so;
    // the geometry of fp8q_quantize_dm_f32 for one row (a resident grid also beyond the caches -- fp8q_quantize_dm_f32 gives every 16 KiB piece its own workgroup there --: the
    // selection prologue is paid once per workgroup: 39.8 us with 6272 workgroups on [64,32,112,112] against 32.7 without it)
    static const int64_t sel_cap = getenv("FP8Q_SEL_CAP") ? atoll(getenv("FP8Q_SEL_CAP")) : kTargetBlocks;
    const RowGrid g = row_grid(1, n, kSmallElems, [](bool nt, int64_t pieces) { return k1_total_cap(nt, pieces, sel_cap); });
    dispatch_k1(g, [&](auto NT, auto U) {
        hipLaunchKernelGGL((k_quant_rows_sel<NT(), U()>), dim3((unsigned)g.bx, 1u), dim3(kBlock), 0, st, x, y, n, sel, si);
    });
    return launch_rc();
}

extern "C" {

int fp8q_copy_f32(const float *x, float *y, int64_t n, fp8q_stream_t stream)
{
    if (!x || !y || n < 0 || (n & 3) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return FP8Q_EINVAL;
    if (n == 0) return FP8Q_OK;
    // K1's grid rule with the copy's own count: a partial last piece is one, and the big-tensor cap goes by the pieces alone
    const RowGrid g = row_grid(1, n, 0, [](bool, int64_t pieces) { return (int64_t)(pieces > 4096 ? 65536 : kTargetBlocks); }, true);
    dispatch<true, false>(g.nt, [&](auto NT) {
        hipLaunchKernelGGL(k_copy<NT()>, dim3((unsigned)g.bx), dim3(kBlock), 0, (hipStream_t)stream, (const vf4 *)x, (vf4 *)y, n / 4);
    });
    return launch_rc();
}

}  // extern "C"
