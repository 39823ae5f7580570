// fp8q_ocp_block.hip -- the hardware FP8 lane under one float32 scale per TILE (gfx950 only): OCP E4M3FN / E5M2 codes of an
// [R, K] tensor (K contiguous) whose scales belong to tiles of 1x128 (activations: along the reduction dimension), 128x1 (the
// operand of a product that reduces over dim 0) or 128x128 (weights) elements -- the operands of a block-scaled FP8 GEMM.
// Tile (i, j) covers rows [tr i, min(tr i + tr, R)) and columns [tk j, min(tk j + tk, K)); edge tiles are short, none wraps.
// The range of a tile is found inside the pass, as in the MX lane; everything after it is fp8q_ocp.hip's arithmetic, from
// fp8q_ocpq.h (one copy for both files; include/fp8q.h states the contract, fp8q_ocp.hip's header derives the redo bound):
//   amax  = the largest bits(|x|) of the tile, compared as unsigned integers: NaN patterns are the largest, then infinity, so
//           the float with those bits is torch.amax(|x|) -- a NaN anywhere in the tile gives NaN, where fmaxf would drop it
//   {scale, 1/scale} = ocp_scale_pair(amax, eps);  code = code4 / code1;  decode = value4 / value_at
// codes are [R, K] in x's own layout for every tile shape, scales float32 [ceil(R / tr), ceil(K / tk)] row-major.
//
// k_ocpb_rows<MODE, F, IN, OUT, NT> -- 1x128 tiles, K % 128 == 0, x and codes / y 16-byte aligned.  The tensor is then a flat
// run of whole tiles.  Lane <-> group of 4 elements (one dword of codes), a tile = the 32 lanes of half a wave, so the range
// is five xor steps (three DPP moves, two shuffles) that never leave the half.  A block takes 4096 elements, wave w the 1024
// from 1024 w on: its four loads, 256 elements apart, are issued before any arithmetic, and every load and store instruction
// of a wave covers one contiguous run (1 KiB of fp32, 512 B of half, 256 B of codes).  The suggested encode geometry -- 16
// consecutive elements per lane, one 16-byte code store -- is k_ocp's and is not taken here: with it a wave's load
// instruction reads 64 pieces of 16 bytes 64 bytes apart; this mapping serves encode and quantize with one kernel body and
// keeps both sides of both contiguous per instruction.  A wave holds 8 consecutive tiles: their scales are gathered into the
// lanes 0..7 and leave as one 32-byte run.
//
// k_ocpb_panel<MODE, F, IN, OUT, TILE, NT> -- 128x1 and 128x128 tiles, K % 4 == 0 and 16-byte aligned pointers.  A workgroup
// of 256 lanes owns a panel of 128 rows x 128 columns and holds it in registers, 64 values per lane, so x is read once.
// Lane t takes the column group t & 31 (4 columns: 16 bytes of fp32, 8 of half) of the rows (t >> 5) + 8 i, i < 16: a wave's
// load instruction reads two whole 512-byte row segments, and all 16 are in flight before the reduction.  Rows past R and
// columns past K (K % 4 == 0: a lane's 4 columns exist together) are +0 in registers -- they cannot change a maximum -- and
// are neither read nor stored, so ragged R and K need no other kernel.
//   128x128: in-lane maximum, six xor steps in the wave, four values through LDS: one scale, stored by lane 0
//   128x1:   in-lane maximum per column, an [8][128] table in LDS (a lane writes its 4 columns as one 16-byte word), lanes
//            0..127 fold the 8 entries of a column, keep {scale, 1/scale} in LDS and store the panel's 128 scales as one
//            512-byte run
// Codes leave as dwords, 4 per lane and row (a wave's store writes two 128-byte row segments); quantize stores values at the
// addresses the elements came from.  Registers, scratch (none) and occupancy of every instantiation:
// profiles/ocp_block_resources.txt.
//
// k_ocpb_plain<MODE, F, IN, OUT> -- everything else (ragged K, misaligned views, row tiles with K % 128 != 0): one wave per
// tile, element by element, two passes over the tile (range, then codes).  The correctness route: the same bytes, no rate is
// claimed for it.
//
// k_ocpb_decode<F, OUT, VEC, NT> -- all three tile shapes: a dword of codes per lane, four a block apart (the store-side
// mapping k_ocp justifies), the scale looked up at [row / tr][col / tk]; VEC needs K % 4 == 0 and 16-byte aligned pointers,
// anything else goes element by element.
// NT: nontemporal loads and stores from 64 MiB of values (kNtBytes), the sibling kernels' rule.  One launch per call, nothing
// read back, no allocation, no workspace.
//
// SR, the trailing template parameter of the three encoding kernels (the fp8q_ocpbsr_* entries; include/fp8q.h states the draw
// and the rounding): code = RNE(SR(q, r)), q by the IEEE division for every element (fp8q_ocpq.h says why), r the draw of the
// element's flat index offset + row K + col in x.  A lane's group of 4 columns starts on a multiple of 4 on the rows and panel
// routes (K % 4 == 0), so it is half a Philox call, drawn where the group is converted -- nothing of it is live across the
// range reduction; the plain route takes one call per element.  SR = false is the kernel as it was, argument block included.
// Registers, scratch (none) and occupancy of both: profiles/ocp_sr_resources.txt.
#include "fp8q_common.h"
#include "fp8q_io.h"
#include "fp8q_mxq.h"       // abs_bits, umax4, umax_xor: the MX lane's integer maxima
#include "fp8q_ocpq.h"

namespace {

enum { kTileRow, kTileCol, kTileFull };     // 1x128, 128x1, 128x128
constexpr int kTile = 128;
constexpr int kRowsChunk = 4096;            // elements of a block of k_ocpb_rows: 4 waves x 4 loads x 64 lanes x 4
constexpr int kPanelLoads = 16;             // rows of a panel per lane

struct OcpbArgs {
    float *scales;          // encode: the scale table, written; decode: read; quantize: null
    int64_t R, K;
    int64_t sK;             // scales per row of the table: ceil(K / tk)
    int64_t panelsC;        // panels (k_ocpb_panel) or tiles (k_ocpb_plain) per row of them
    int64_t tiles;          // k_ocpb_plain: tiles in all
    int tr, tk;             // the tile
    int kind;               // kTile*
    int small;              // R * K < 2^31: decode divides in 32 bits
    float eps;
};

// the SR kernels' argument block: OcpbArgs and the call's seed and offset
struct OcpbSrArgs : OcpbArgs {
    MxSr sr;
};
template <bool SR>
using OcpbArgsOf = std::conditional_t<SR, OcpbSrArgs, OcpbArgs>;

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

template <int STEP>
__device__ __forceinline__ uint32_t umax_shfl(uint32_t m)
{
    return umax(m, (uint32_t)__shfl_xor((int)m, STEP));
}

// ---- 1x128 tiles of a flat run of whole tiles ----
template <int MODE, int F, class IN, class OUT, bool NT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_ocpb_rows(const void *__restrict__ in, void *__restrict__ out, OcpbArgsOf<SR> a)
{
    typedef typename IN::elem in_t;
    typedef typename OUT::elem out_t;
    const in_t *x = static_cast<const in_t *>(in);
    out_t *y = static_cast<out_t *>(out);
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t n = a.R * a.K;
    const int64_t base = (int64_t)blockIdx.x * kRowsChunk + (tid >> 6) * (kRowsChunk / 4);
    float v[4][4];
    bool live[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t e = base + u * 256 + 4 * lane;
        live[u] = e < n;                       // n is a multiple of 128: a tile (half a wave) is there or is not
        v[u][0] = v[u][1] = v[u][2] = v[u][3] = 0.0f;
        if (live[u]) IN::template load4<NT>(x + e, v[u]);
    }
    float sc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        uint32_t m = umax4(v[u]);
        m = umax_xor<1>(m);
        m = umax_xor<2>(m);
        m = umax_xor<4>(m);
        m = umax_shfl<8>(m);
        m = umax_shfl<16>(m);
        const float4 k = ocp_scale_pair<F>(__uint_as_float(m), a.eps);
        const float4 k4[4] = {k, k, k, k};
        const int64_t e = base + u * 256 + 4 * lane;
        uint32_t w;
        if constexpr (SR) w = code4_sr_at<F>(a.sr, v[u], k4, e);
        else w = code4<F>(v[u], k4);
        sc[u] = k.x;
        if constexpr (MODE == kEncode) {
            if (live[u]) stv<NT>(reinterpret_cast<uint32_t *>(y + e), w);
        } else {
            float r[4];
            value4<F>(w, k4, r);
            if (live[u]) OUT::template store4<NT>(y + e, r);
        }
    }
    if constexpr (MODE == kEncode) {
        // tile j of the wave's 8 is held by the half j & 1 of load j >> 1: into lane j, then one 32-byte run
        float mine = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float s = __shfl(sc[j >> 1], 32 * (j & 1));
            if (lane == j) mine = s;
        }
        const int64_t t0 = base >> 7;
        if (lane < 8 && t0 + lane < (n >> 7)) a.scales[t0 + lane] = mine;
    }
}

// ---- 128x1 and 128x128 tiles: a panel of 128 x 128 per workgroup, in registers ----
template <int MODE, int F, class IN, class OUT, int TILE, bool NT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_ocpb_panel(const void *__restrict__ in, void *__restrict__ out, OcpbArgsOf<SR> a)
{
    typedef typename IN::elem in_t;
    typedef typename OUT::elem out_t;
    __shared__ __attribute__((aligned(16))) uint32_t s_m[TILE == kTileCol ? 8 * kTile : 4];
    __shared__ float2 s_k[TILE == kTileCol ? kTile : 1];
    const in_t *x = static_cast<const in_t *>(in);
    out_t *y = static_cast<out_t *>(out);
    const int tid = threadIdx.x, cg = tid & 31, rr = tid >> 5;
    const int64_t pr = (int64_t)blockIdx.x / a.panelsC, pc = (int64_t)blockIdx.x - pr * a.panelsC;
    const int64_t r0 = pr * kTile + rr, c0 = pc * kTile, c = c0 + 4 * cg;
    const bool col_live = c < a.K;
    float v[kPanelLoads][4];
#pragma unroll
    for (int i = 0; i < kPanelLoads; ++i) {
        v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.0f;
        const int64_t row = r0 + 8 * i;
        if (col_live && row < a.R) IN::template load4<NT>(x + row * a.K + c, v[i]);
    }
    float4 k4[4];
    if constexpr (TILE == kTileFull) {
        uint32_t m = 0u;
#pragma unroll
        for (int i = 0; i < kPanelLoads; ++i) m = umax(m, umax4(v[i]));
        m = umax_xor<1>(m);
        m = umax_xor<2>(m);
        m = umax_xor<4>(m);
        m = umax_shfl<8>(m);
        m = umax_shfl<16>(m);
        m = umax_shfl<32>(m);
        if ((tid & 63) == 0) s_m[tid >> 6] = m;
        __syncthreads();
        m = umax(umax(s_m[0], s_m[1]), umax(s_m[2], s_m[3]));
        const float4 k = ocp_scale_pair<F>(__uint_as_float(m), a.eps);
        if (MODE == kEncode && tid == 0) a.scales[pr * a.sK + pc] = k.x;
        k4[0] = k4[1] = k4[2] = k4[3] = k;
    } else {
        uint32_t mc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < kPanelLoads; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) mc[j] = umax(mc[j], abs_bits(v[i][j]));
        }
        *reinterpret_cast<u4v *>(s_m + rr * kTile + 4 * cg) = u4v{mc[0], mc[1], mc[2], mc[3]};
        __syncthreads();
        if (tid < kTile) {
            uint32_t m = s_m[tid];
#pragma unroll
            for (int q = 1; q < 8; ++q) m = umax(m, s_m[q * kTile + tid]);
            const float4 k = ocp_scale_pair<F>(__uint_as_float(m), a.eps);
            s_k[tid] = make_float2(k.x, k.y);
            if (MODE == kEncode && c0 + tid < a.K) a.scales[pr * a.sK + c0 + tid] = k.x;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 k = s_k[4 * cg + j];
            k4[j] = make_float4(k.x, k.y, 0.0f, 0.0f);
        }
    }
#pragma unroll
    for (int i = 0; i < kPanelLoads; ++i) {
        const int64_t row = r0 + 8 * i;
        uint32_t w;
        if constexpr (SR) w = code4_sr_at<F>(a.sr, v[i], k4, row * a.K + c);
        else w = code4<F>(v[i], k4);
        if constexpr (MODE == kEncode) {
            if (col_live && row < a.R) stv<NT>(reinterpret_cast<uint32_t *>(y + row * a.K + c), w);
        } else {
            float r[4];
            value4<F>(w, k4, r);
            if (col_live && row < a.R) OUT::template store4<NT>(y + row * a.K + c, r);
        }
    }
}

// ---- the general route: one wave per tile, element by element ----
template <int MODE, int F, class IN, class OUT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_ocpb_plain(const void *__restrict__ in, void *__restrict__ out, OcpbArgsOf<SR> a)
{
    typedef typename IN::elem in_t;
    typedef typename OUT::elem out_t;
    const in_t *x = static_cast<const in_t *>(in);
    out_t *y = static_cast<out_t *>(out);
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (t >= a.tiles) return;                  // the whole wave: nothing below synchronises the block
    const int64_t ti = t / a.panelsC, tj = t - ti * a.panelsC;
    const int64_t r0 = ti * a.tr, c0 = tj * a.tk;
    const int h = (int)(a.R - r0 < a.tr ? a.R - r0 : a.tr), wd = (int)(a.K - c0 < a.tk ? a.K - c0 : a.tk);
    const int n = h * wd;
    uint32_t m = 0u;
    for (int e = lane; e < n; e += 64) {
        const int i = e / wd, j = e - i * wd;
        m = umax(m, abs_bits(IN::load1(x + (r0 + i) * a.K + c0 + j)));
    }
    m = umax_xor<1>(m);
    m = umax_xor<2>(m);
    m = umax_xor<4>(m);
    m = umax_shfl<8>(m);
    m = umax_shfl<16>(m);
    m = umax_shfl<32>(m);
    const float4 k = ocp_scale_pair<F>(__uint_as_float(m), a.eps);
    if (MODE == kEncode && lane == 0) a.scales[t] = k.x;
    for (int e = lane; e < n; e += 64) {
        const int i = e / wd, j = e - i * wd;
        const int64_t at = (r0 + i) * a.K + c0 + j;
        uint32_t code;
        if constexpr (SR) code = code1_sr<F>(IN::load1(x + at), k, mx_draw1(a.sr, a.sr.offset + (uint64_t)at));
        else code = code1<F>(IN::load1(x + at), k);
        if constexpr (MODE == kEncode) y[at] = (uint8_t)code;
        else OUT::store1(y + at, value_at<F, 0>(code, k.x));
    }
}

// ---- decode: every tile shape ----
// the scale of element (row, col); the four elements of a group share a row, and under 128-wide tiles a scale
__device__ __forceinline__ int64_t scale_at(const OcpbArgs &a, int64_t row, int64_t col)
{
    if (a.kind == kTileRow) return row * a.sK + (col >> 7);
    if (a.kind == kTileCol) return (row >> 7) * a.sK + col;
    return (row >> 7) * a.sK + (col >> 7);
}

__device__ __forceinline__ void row_col(const OcpbArgs &a, int64_t e, int64_t &row, int64_t &col)
{
    if (a.small) row = (int64_t)((uint32_t)e / (uint32_t)a.K);
    else row = e / a.K;
    col = e - row * a.K;
}

template <int F, class OUT, bool VEC, bool NT>
__global__ void __launch_bounds__(kBlock)
k_ocpb_decode(const uint8_t *__restrict__ codes, void *__restrict__ out, OcpbArgs a)
{
    typedef typename OUT::elem out_t;
    out_t *y = static_cast<out_t *>(out);
    const float *scales = a.scales;
    const int64_t n = a.R * a.K;
    if constexpr (VEC) {
        const int64_t g0 = (int64_t)blockIdx.x * (4 * kBlock) + threadIdx.x;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t e = 4 * (g0 + u * kBlock);
            if (e < n) w[u] = IoCodes::load4<NT>(codes + e);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t e = 4 * (g0 + u * kBlock);
            if (e >= n) continue;
            int64_t row, col;
            row_col(a, e, row, col);
            const int64_t at = scale_at(a, row, col);
            const float s0 = scales[at];
            float4 k4[4];
            k4[0] = k4[1] = k4[2] = k4[3] = make_float4(s0, 0.0f, 0.0f, 0.0f);
            if (a.kind == kTileCol) {
                k4[1].x = scales[at + 1];
                k4[2].x = scales[at + 2];
                k4[3].x = scales[at + 3];
            }
            float r[4];
            value4<F>(w[u], k4, r);
            OUT::template store4<NT>(y + e, r);
        }
    } else {
        const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (e >= n) return;
        int64_t row, col;
        row_col(a, e, row, col);
        OUT::store1(y + e, value_at<F, 0>(codes[e], scales[scale_at(a, row, col)]));
    }
}

// ---- host side ----
inline int tile_kind(int tr, int tk)
{
    if (tr == 1 && tk == kTile) return kTileRow;
    if (tr == kTile && tk == 1) return kTileCol;
    if (tr == kTile && tk == kTile) return kTileFull;
    return -1;
}

// THE launch rule of encode and quantize: which kernel an [R, K] tensor under (tr, tk) tiles takes
int ocpb_route(int64_t R, int64_t K, int tr, int tk, int x_type, int aligned16)
{
    if (R <= 0 || K <= 0 || R > INT64_MAX / K) return FP8Q_EINVAL;
    const int kind = tile_kind(tr, tk);
    if (kind < 0) return FP8Q_EUNSUPPORTED;
    if (x_type != FP8Q_DT_F32 && !half_type(x_type)) return FP8Q_EINVAL;
    if (!aligned16) return FP8Q_OCPB_PLAIN;
    if (kind == kTileRow) return K % kTile == 0 ? FP8Q_OCPB_ROWS : FP8Q_OCPB_PLAIN;
    return K % 4 == 0 ? FP8Q_OCPB_PANEL : FP8Q_OCPB_PLAIN;
}

// Argument checks (everything is reported before the launch) and the one launch.  in_type / out_type: FP8Q_DT_* of the value
// side(s), -1 for the side that holds codes.  scales: encode's output, decode's input, null for quantize.  sr: the seed and
// offset of a stochastic-rounding entry (encode, quantize), null for round to nearest even.
int ocpb_launch(int mode, const void *in, void *out, float *scales, int in_type, int out_type, int64_t R, int64_t K, int tr,
                int tk, int fmt, float eps, hipStream_t st, const MxSr *sr = nullptr)
{
    if (!in || !out || (mode != kQuant && !scales) || R <= 0 || K <= 0 || R > INT64_MAX / K) return FP8Q_EINVAL;
    const int kind = tile_kind(tr, tk);
    if ((fmt != FP8Q_OCP_E4M3FN && fmt != FP8Q_OCP_E5M2) || kind < 0) return FP8Q_EUNSUPPORTED;
    if (value_side_misaligned(in, in_type) || value_side_misaligned(out, out_type) || ((uintptr_t)scales & 3))
        return FP8Q_EINVAL;
    if (sr && (sr->offset & 7u)) return FP8Q_EINVAL;
    const bool aligned16 = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const int64_t n = R * K;
    const bool nt = n >= kNtBytes / 4;
    OcpbSrArgs a = {};
    if (sr) a.sr = *sr;
    a.scales = scales;
    a.R = R;
    a.K = K;
    a.sK = cdiv(K, tk);
    a.tr = tr;
    a.tk = tk;
    a.kind = kind;
    a.small = n < ((int64_t)1 << 31);
    a.eps = eps;
    int route;
    int64_t grid;
    if (mode == kDecode) {
        route = aligned16 && K % 4 == 0;        // (decode has two kernels of its own: by dwords, or element by element)
        grid = route ? cdiv(n, 16 * kBlock) : cdiv(n, kBlock);
    } else {
        route = ocpb_route(R, K, tr, tk, FP8Q_DT_F32, aligned16);
        if (route == FP8Q_OCPB_ROWS) {
            grid = cdiv(n, kRowsChunk);
        } else if (route == FP8Q_OCPB_PANEL) {
            a.panelsC = cdiv(K, kTile);
            const int64_t pr = cdiv(R, kTile);
            grid = pr > (int64_t)INT32_MAX / a.panelsC ? (int64_t)INT32_MAX + 1 : pr * a.panelsC;
        } else {
            a.panelsC = a.sK;
            const int64_t tiR = cdiv(R, tr);
            if (tiR > INT64_MAX / a.panelsC) return FP8Q_EINVAL;
            a.tiles = tiR * a.panelsC;
            grid = cdiv(a.tiles, kBlock / 64);
        }
    }
    if (grid > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    const dim3 g((unsigned)grid), b(kBlock);
    io_dispatch(mode, in_type, out_type, [&](auto m, auto ti, auto to) {
        constexpr int MODE = decltype(m)::value;
        typedef decltype(ti) IN;
        typedef decltype(to) OUT;
        dispatch<FP8Q_OCP_E4M3FN, FP8Q_OCP_E5M2>(fmt, [&](auto fc) {
            constexpr int F = decltype(fc)::value;
            if constexpr (MODE == kDecode) {
                const uint8_t *c = static_cast<const uint8_t *>(in);
                const OcpbArgs &ad = a;
                if (!route) hipLaunchKernelGGL((k_ocpb_decode<F, OUT, false, false>), g, b, 0, st, c, out, ad);
                else if (nt) hipLaunchKernelGGL((k_ocpb_decode<F, OUT, true, true>), g, b, 0, st, c, out, ad);
                else hipLaunchKernelGGL((k_ocpb_decode<F, OUT, true, false>), g, b, 0, st, c, out, ad);
            } else {
                dispatch<true, false>(sr != nullptr, [&](auto src) {
                    constexpr bool SR = decltype(src)::value;
                    const OcpbArgsOf<SR> &as = a;       // (the round-to-nearest-even kernels take the OcpbArgs part)
                    if (route == FP8Q_OCPB_PLAIN) {
                        hipLaunchKernelGGL((k_ocpb_plain<MODE, F, IN, OUT, SR>), g, b, 0, st, in, out, as);
                        return;
                    }
                    dispatch<true, false>(nt, [&](auto ntc) {
                        constexpr bool NT = decltype(ntc)::value;
                        if (route == FP8Q_OCPB_ROWS)
                            hipLaunchKernelGGL((k_ocpb_rows<MODE, F, IN, OUT, NT, SR>), g, b, 0, st, in, out, as);
                        else if (kind == kTileCol)
                            hipLaunchKernelGGL((k_ocpb_panel<MODE, F, IN, OUT, kTileCol, NT, SR>), g, b, 0, st, in, out, as);
                        else
                            hipLaunchKernelGGL((k_ocpb_panel<MODE, F, IN, OUT, kTileFull, NT, SR>), g, b, 0, st, in, out, as);
                    });
                });
            }
        });
    });
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_ocpb_route(int64_t R, int64_t K, int tile_r, int tile_k, int x_type, int aligned16)
{
    return ocpb_route(R, K, tile_r, tile_k, x_type, aligned16);
}

int fp8q_ocpb_encode_f32(const float *x, uint8_t *codes, float *scales, int64_t R, int64_t K, int tile_r, int tile_k, int fmt,
                         float eps, fp8q_stream_t stream)
{
    return ocpb_launch(kEncode, x, codes, scales, FP8Q_DT_F32, -1, R, K, tile_r, tile_k, fmt, eps, (hipStream_t)stream);
}

int fp8q_ocpb_encode_h16(const void *x, uint8_t *codes, float *scales, int x_type, int64_t R, int64_t K, int tile_r, int tile_k,
                         int fmt, float eps, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    return ocpb_launch(kEncode, x, codes, scales, x_type, -1, R, K, tile_r, tile_k, fmt, eps, (hipStream_t)stream);
}

int fp8q_ocpb_decode_f32(const uint8_t *codes, const float *scales, float *y, int64_t R, int64_t K, int tile_r, int tile_k,
                         int fmt, fp8q_stream_t stream)
{
    return ocpb_launch(kDecode, codes, y, const_cast<float *>(scales), -1, FP8Q_DT_F32, R, K, tile_r, tile_k, fmt, 0.0f,
                       (hipStream_t)stream);
}

int fp8q_ocpb_decode_h16(const uint8_t *codes, const float *scales, void *y, int y_type, int64_t R, int64_t K, int tile_r,
                         int tile_k, int fmt, fp8q_stream_t stream)
{
    if (!half_type(y_type)) return FP8Q_EINVAL;
    return ocpb_launch(kDecode, codes, y, const_cast<float *>(scales), -1, y_type, R, K, tile_r, tile_k, fmt, 0.0f,
                       (hipStream_t)stream);
}

int fp8q_ocpb_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int tile_r, int tile_k, int fmt, float eps,
                           fp8q_stream_t stream)
{
    return ocpb_launch(kQuant, x, y, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, tile_r, tile_k, fmt, eps, (hipStream_t)stream);
}

int fp8q_ocpb_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int tile_r, int tile_k,
                           int fmt, float eps, fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    return ocpb_launch(kQuant, x, y, nullptr, x_type, y_type, R, K, tile_r, tile_k, fmt, eps, (hipStream_t)stream);
}

int fp8q_ocpbsr_encode_f32(const float *x, uint8_t *codes, float *scales, int64_t R, int64_t K, int tile_r, int tile_k, int fmt,
                           float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return ocpb_launch(kEncode, x, codes, scales, FP8Q_DT_F32, -1, R, K, tile_r, tile_k, fmt, eps, (hipStream_t)stream, &sr);
}

int fp8q_ocpbsr_encode_h16(const void *x, uint8_t *codes, float *scales, int x_type, int64_t R, int64_t K, int tile_r,
                           int tile_k, int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    const MxSr sr = mx_sr_args(seed, offset);
    return ocpb_launch(kEncode, x, codes, scales, x_type, -1, R, K, tile_r, tile_k, fmt, eps, (hipStream_t)stream, &sr);
}

int fp8q_ocpbsr_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int tile_r, int tile_k, int fmt, float eps,
                             uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return ocpb_launch(kQuant, x, y, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, tile_r, tile_k, fmt, eps, (hipStream_t)stream,
                       &sr);
}

int fp8q_ocpbsr_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int tile_r, int tile_k,
                             int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    const MxSr sr = mx_sr_args(seed, offset);
    return ocpb_launch(kQuant, x, y, nullptr, x_type, y_type, R, K, tile_r, tile_k, fmt, eps, (hipStream_t)stream, &sr);
}

}  // extern "C"
