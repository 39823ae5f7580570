// fp8q_ocp_block_t.hip -- the tile-scaled hardware FP8 lane with the operands TRANSPOSED (gfx950 only): the block-scaled
// operands of x^T made from x as it lies, for the two backward products, which reduce over dim 0 (dx = dy . W, dW = dy^T . x).
// x is [R, K], K contiguous.  By reference (include/fp8q.h): the transposed operands are, byte for byte, what fp8q_ocp_block.hip
// gives for the contiguous [K, R] tensor x^T under the same tile,
//   encode_t     codes_t [K, R] and scales_t float32 [K, ceil(R / 128)] for (1, 128), [ceil(K / 128), ceil(R / 128)] for (128, 128)
//   encode_both  the row-wise operands of fp8q_ocpb_encode_* and the transposed ones, from one read of x
// (1, 128): the two halves of encode_both are two quantizations (row tiles and column tiles have their own scales); (128, 128):
// one quantization stored twice.  (128, 1) is refused: its result would be x's 1x128 quantization with transposed codes, the
// operand of no product.  The arithmetic is fp8q_ocpq.h's (ocp_scale_pair, code4, code1), the integer maxima fp8q_mxq.h's; a
// code does not depend on which three elements share its code4 call (where the two ends of a word agree every byte is the
// contract's code, where they do not every byte is redone by the division), so codes may be grouped along either axis.
//
// k_ocpbt_panel<OP, F, IN, TILE, NT> -- K % 4 == 0 and every pointer of the call 16-byte aligned.  A workgroup of 256 lanes owns a
// panel of 128 rows x 128 columns and holds it in registers, 64 values per lane; all 16 loads are issued before any arithmetic.
//   lane <-> (rg = tid / 32, cg = tid % 32): the 16 consecutive rows 16 rg .. 16 rg + 15 of the 4 columns 4 cg .. 4 cg + 3 (16
//           bytes of fp32, 8 of half).  k_ocpb_panel's lanes hold rows 8 apart; here the codes of one column of one lane are 16
//           contiguous bytes of a codes_t row, packed in registers.  A wave is the row groups 2w and 2w + 1: its load
//           instruction still reads two whole row segments (512 bytes of fp32, 256 of half).  Rows past R and columns past K
//           (K % 4 == 0: a lane's 4 columns exist together) are +0 in registers and are neither read nor stored.
//   ranges: (128, 128) in-lane maximum, six xor steps, four values through LDS, as k_ocpb_panel<kTileFull>; (1, 128) in-lane
//           maximum per column over the 16 rows, an [8][128] table in LDS (a lane writes its 4 columns as one 16-byte word), lanes
//           0..127 fold a column's 8 entries and keep {scale, 1/scale} in LDS, as k_ocpb_panel<kTileCol>.  encode_both at (1, 128)
//           also needs the row maxima: a row's 128 columns are the 32 lanes of half a wave, so five xor steps (three DPP moves,
//           two shuffles) that never leave the half, as k_ocpb_rows; the row-wise half is converted and stored FIRST, row by row,
//           so nothing of it is live while the transposed half is converted.
//   row-wise codes (encode_both) leave as dwords from the lanes that hold them: a wave's store writes two 128-byte row segments.
//   (128, 128): the codes are made once, row-wise, and the transposed words are a 4x4 byte transposition in registers.
//   transposed codes go through LDS -- codes, not values: 16 KiB of payload per panel -- and leave along R: a column's 128 rows
//           are 128 contiguous bytes of codes_t, 8 consecutive lanes store them as 16-byte words, so a wave's store instruction
//           covers 8 whole runs.  16-byte words need R % 16 == 0, dwords R % 4 == 0, anything else goes byte by byte
//           (fp8q_ocpbt_route reports which).  The width divides 128 and R, hence the rows of every panel, the short last one
//           included: there is no short last word to treat apart.
//   scales_t at (1, 128): a panel has one scale per column, ceil(R / 128) floats apart: isolated 4-byte stores, which the MX
//           lane measured at about 32 bytes of traffic each (profiles/mx_t_pmc.txt).  That is about 4 KiB per panel next to the
//           80 KiB of values and codes, and it is left so; the row-wise scales of encode_both are the same case.
// LDS layout of the codes and its bank conflicts, by the per-instruction rules (ds_write_b32 and ds_read_b32: the lanes 0..31 and
// 32..63 are serviced apart, bank = (byte address / 4) mod 32).  The [column][run + 4 bytes] image of fp8q_mx_t.hip does not
// carry over: there 16 lanes of a half-wave step 4 columns apart; here 32 lanes do, 4 x pitch x cg mod 32 takes 8 values at
// most whatever the pitch, so every write would be 4-way.  So the image is kept in the order the WRITERS hold it, and the
// readers untangle it: lane (rg, cg) owns a block of 16 dwords, dword 4 j + h = its rows 4 h .. 4 h + 3 of its column j, at
//       dword rg * kGroupPitch + cg * kLanePitch,   kLanePitch = 17,   kGroupPitch = 32 * 17 + 5 = 549   (17568 bytes in all)
//   writes, 16 dword stores per lane: a half-wave is one rg and cg = 0..31, its banks are 17 cg + const mod 32 -- 17 is odd, all
//           32 differ: conflict-free.
//   reads, 16-byte route, four dword loads per word: lane u of a pass takes the column u / 8, rows 16 (u % 8) ..: a half-wave is
//           4 columns of one cg (j = 0..3) x rg = 0..7, and dword d of them sits at bank 549 rg + 4 j + d + const = 5 rg + 4 j +
//           const mod 32.  5 drg = 4 dj mod 32 with |drg| <= 7, |dj| <= 3 has the solutions (drg, dj) = +-(4, -3) only (5^-1 =
//           13 mod 32: drg = 20 dj), and no three points are pairwise 4 apart in rg: 2-way, which the four waves' alternating
//           issue covers.  (A group pitch of 0 mod 32 would make the 8 row groups of a column meet on one bank, 1 mod 32 would
//           do here but is 4-way on the dword route.)
//   reads, dword route: a half-wave is one column, rg = 0..7 x d = 0..3, bank 5 rg + d + const: 5 drg = dd mod 32 with |dd| <= 3
//           gives (drg, dd) = +-(-6, 2), +-(7, 3), never three at once: 2-way.  Byte route: four lanes share a dword, the 8
//           dwords of a half-wave are 2 row groups x 4, banks 5 rg + d: conflict-free.
// The LDS moves 1 byte per element against 4 + 1 (fp32) of HBM traffic; none of this is near a limit.
//
// k_ocpbt_plain<OP, F, IN, TILE> -- everything else (K % 4 != 0, misaligned views): one wave per transposed tile, element by
// element, two passes over the tile, the same bytes.  (128, 128) writes both orientations from the wave that has the tile;
// encode_both at (1, 128) gives the row tiles waves of their own, so that route reads x twice.  The correctness route: no rate
// is claimed for it.
// NT: nontemporal loads and stores from 64 MiB of values (kNtBytes), the lane's rule.  One launch per call, nothing read back, no
// allocation, no workspace.  Registers, scratch (none) and occupancy of every instantiation: profiles/ocp_block_t_resources.txt.
// gfx950's scaled conversions are not used, for the reason fp8q_ocp.hip gives.
//
// SR, the trailing template parameter of both kernels (the fp8q_ocpbtsr_* entries; include/fp8q.h states the draw and the
// rounding): code = RNE(SR(q, r)), q by the IEEE division for every element (fp8q_ocpq.h says why), r the draw of the element's
// flat index offset + row K + col in x AS IT LIES, whichever orientation the code is stored in.  On the panel route a lane's 4
// columns of one row are an aligned group of four flat indices, half a Philox call.  (128, 128): the codes are still made once,
// row-wise, each word under its row's draws.  (1, 128): a transposed word holds one column of four ROWS, so the draws of the
// four rows 4 h .. 4 h + 3 (four half calls, 16 draws) are made once per h and serve the lane's four columns -- the loop runs h
// outside, j inside, where the kernel without SR runs j outside.  encode_both converts and stores the row-wise half first and
// draws again for the transposed half (the same draws: the draw belongs to the element), so the 32 words of a lane's draws are
// never held next to its 64 values.  The plain route takes one call per element.  SR = false is the kernel as it was,
// argument block included.  Registers, scratch (none) and occupancy of both: profiles/ocp_sr_resources.txt.
#include "fp8q_common.h"
#include "fp8q_io.h"
#include "fp8q_mxq.h"       // abs_bits, umax4, umax_xor: the MX lane's integer maxima
#include "fp8q_ocpq.h"

namespace {

enum { kOpT, kOpBoth };                 // encode_t, encode_both
enum { kTileRow, kTileFull };           // 1x128 (of x^T: 128 rows of one column of x), 128x128
constexpr int kTile = 128;
constexpr int kLaneRows = 16;           // consecutive rows of a panel per lane
constexpr int kLanePitch = 17;          // dwords from one lane's block of codes to the next in LDS
constexpr int kGroupPitch = 32 * kLanePitch + 5;    // and from one row group's blocks to the next

struct OcpbtArgs {
    uint8_t *codes, *codes_t;           // the row-wise codes (encode_both), the transposed ones
    float *scales, *scales_t;
    int64_t R, K;
    int64_t nR, nK;                     // ceil(R / 128), ceil(K / 128)
    int64_t tiles_t, tiles;             // k_ocpbt_plain: transposed tiles, all tiles
    int tkw;                            // k_ocpbt_plain: columns of x under a transposed tile, 1 or 128
    int gran;                           // bytes per store of transposed codes: 16, 4 or 1
    float eps;
};

// the SR kernels' argument block: OcpbtArgs and the call's seed and offset
struct OcpbtSrArgs : OcpbtArgs {
    MxSr sr;
};
template <bool SR>
using OcpbtArgsOf = std::conditional_t<SR, OcpbtSrArgs, OcpbtArgs>;

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

template <int STEP>
__device__ __forceinline__ uint32_t umax_shfl(uint32_t m)
{
    return umax(m, (uint32_t)__shfl_xor((int)m, STEP));
}

// one panel's transposed codes from LDS (s) to codes_t (dst: the panel's first byte), G bytes per store; run: the rows of the
// panel that are rows of the tensor (a multiple of G), ncols: the columns that are
template <int G, bool NT>
__device__ __forceinline__ void store_runs(const uint32_t *s, uint8_t *dst, int64_t pitch, int run, int ncols, int tid)
{
    constexpr int UPC = kTile / G;              // stores per column of a full panel
    for (int u = tid; u < kTile * UPC; u += kBlock) {
        const int col = u / UPC, off = (u - col * UPC) * G;
        if (col >= ncols || off >= run) continue;
        // byte `off` of column col: the block of lane (off / 16, col / 4), dword 4 (col % 4) + (off % 16) / 4
        const uint32_t *src = s + (off >> 4) * kGroupPitch + (col >> 2) * kLanePitch + 4 * (col & 3) + ((off >> 2) & 3);
        uint8_t *d = dst + col * pitch + off;
        if constexpr (G == 16) stv<NT>(reinterpret_cast<u4v *>(d), u4v{src[0], src[1], src[2], src[3]});
        else if constexpr (G == 4) stv<NT>(reinterpret_cast<uint32_t *>(d), src[0]);
        else *d = (uint8_t)(src[0] >> (8 * (off & 3)));
    }
}

// ---- the panel route ----
template <int OP, int F, class IN, int TILE, bool NT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_ocpbt_panel(const void *__restrict__ in, OcpbtArgsOf<SR> a)
{
    typedef typename IN::elem in_t;
    __shared__ uint32_t s_codes[8 * kGroupPitch];
    __shared__ __attribute__((aligned(16))) uint32_t s_m[TILE == kTileRow ? 8 * kTile : 4];
    __shared__ float2 s_k[TILE == kTileRow ? kTile : 1];
    const in_t *x = static_cast<const in_t *>(in);
    const int tid = threadIdx.x, cg = tid & 31, rg = tid >> 5;
    const int64_t pr = (int64_t)blockIdx.x / a.nK, pc = (int64_t)blockIdx.x - pr * a.nK;
    const int64_t r0 = pr * kTile, c0 = pc * kTile;
    const int64_t row0 = r0 + kLaneRows * rg, c = c0 + 4 * cg;
    const bool col_live = c < a.K;
    float v[kLaneRows][4];
#pragma unroll
    for (int i = 0; i < kLaneRows; ++i) {
        v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.0f;
        if (col_live && row0 + i < a.R) IN::template load4<NT>(x + (row0 + i) * a.K + c, v[i]);
    }
    uint32_t *mine = s_codes + rg * kGroupPitch + cg * kLanePitch;      // dword 4 j + h: rows 4 h .. 4 h + 3 of column j
    if constexpr (TILE == kTileFull) {
        uint32_t m = 0u;
#pragma unroll
        for (int i = 0; i < kLaneRows; ++i) m = umax(m, umax4(v[i]));
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
        if (tid == 0) {
            a.scales_t[pc * a.nR + pr] = k.x;
            if constexpr (OP == kOpBoth) a.scales[pr * a.nK + pc] = k.x;
        }
        const float4 k4[4] = {k, k, k, k};
        // one quantization: the row-wise words, and their 4x4 byte transpositions for the other orientation
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            uint32_t w[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int i = 4 * h + p;
                if constexpr (SR) w[p] = code4_sr_at<F>(a.sr, v[i], k4, (row0 + i) * a.K + c);
                else w[p] = code4<F>(v[i], k4);
                if constexpr (OP == kOpBoth) {
                    const int64_t row = row0 + i;
                    if (col_live && row < a.R) stv<NT>(reinterpret_cast<uint32_t *>(a.codes + row * a.K + c), w[p]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                mine[4 * j + h] = ((w[0] >> (8 * j)) & 0xffu) | (((w[1] >> (8 * j)) & 0xffu) << 8) |
                                  (((w[2] >> (8 * j)) & 0xffu) << 16) | (((w[3] >> (8 * j)) & 0xffu) << 24);
        }
    } else {
        uint32_t mc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < kLaneRows; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) mc[j] = umax(mc[j], abs_bits(v[i][j]));
        }
        *reinterpret_cast<u4v *>(s_m + rg * kTile + 4 * cg) = u4v{mc[0], mc[1], mc[2], mc[3]};
        __syncthreads();
        if (tid < kTile) {
            uint32_t m = s_m[tid];
#pragma unroll
            for (int q = 1; q < 8; ++q) m = umax(m, s_m[q * kTile + tid]);
            const float4 k = ocp_scale_pair<F>(__uint_as_float(m), a.eps);
            s_k[tid] = make_float2(k.x, k.y);
            if (c0 + tid < a.K) a.scales_t[(c0 + tid) * a.nR + pr] = k.x;
        }
        if constexpr (OP == kOpBoth) {
            // the row-wise half, first: every lane of the wave runs the folds
#pragma unroll
            for (int i = 0; i < kLaneRows; ++i) {
                uint32_t m = umax4(v[i]);
                m = umax_xor<1>(m);
                m = umax_xor<2>(m);
                m = umax_xor<4>(m);
                m = umax_shfl<8>(m);
                m = umax_shfl<16>(m);
                const float4 k = ocp_scale_pair<F>(__uint_as_float(m), a.eps);
                const float4 k4[4] = {k, k, k, k};
                const int64_t row = row0 + i;
                uint32_t w;
                if constexpr (SR) w = code4_sr_at<F>(a.sr, v[i], k4, row * a.K + c);
                else w = code4<F>(v[i], k4);
                if (row < a.R) {
                    if (col_live) stv<NT>(reinterpret_cast<uint32_t *>(a.codes + row * a.K + c), w);
                    if (cg == 0) a.scales[row * a.nK + pc] = k.x;
                }
            }
        }
        __syncthreads();
        if constexpr (SR) {
            float4 kc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 kj = s_k[4 * cg + j];
                kc[j] = make_float4(kj.x, kj.y, 0.0f, 0.0f);
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                uint32_t r[4][4];               // [row 4 h + p][column j]
#pragma unroll
                for (int p = 0; p < 4; ++p) sr_draws4(a.sr, a.sr.offset + (uint64_t)((row0 + 4 * h + p) * a.K + c), r[p]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 k4[4] = {kc[j], kc[j], kc[j], kc[j]};
                    const float t[4] = {v[4 * h][j], v[4 * h + 1][j], v[4 * h + 2][j], v[4 * h + 3][j]};
                    const uint32_t rt[4] = {r[0][j], r[1][j], r[2][j], r[3][j]};
                    mine[4 * j + h] = code4_sr<F>(t, k4, rt);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 kj = s_k[4 * cg + j];
                const float4 k = make_float4(kj.x, kj.y, 0.0f, 0.0f);
                const float4 k4[4] = {k, k, k, k};
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const float t[4] = {v[4 * h][j], v[4 * h + 1][j], v[4 * h + 2][j], v[4 * h + 3][j]};
                    mine[4 * j + h] = code4<F>(t, k4);
                }
            }
        }
    }
    __syncthreads();
    const int run = (int)(a.R - r0 < kTile ? a.R - r0 : kTile);
    const int ncols = (int)(a.K - c0 < kTile ? a.K - c0 : kTile);
    uint8_t *dst = a.codes_t + c0 * a.R + r0;
    if (a.gran == 16) store_runs<16, NT>(s_codes, dst, a.R, run, ncols, tid);
    else if (a.gran == 4) store_runs<4, NT>(s_codes, dst, a.R, run, ncols, tid);
    else store_runs<1, NT>(s_codes, dst, a.R, run, ncols, tid);
}

// ---- the general route: one wave per tile, element by element ----
template <int OP, int F, class IN, int TILE, bool SR>
__global__ void __launch_bounds__(kBlock)
k_ocpbt_plain(const void *__restrict__ in, OcpbtArgsOf<SR> a)
{
    typedef typename IN::elem in_t;
    const in_t *x = static_cast<const in_t *>(in);
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (t >= a.tiles) return;                  // the whole wave: nothing below synchronises the block
    const bool rowwise = t >= a.tiles_t;       // the row tiles of encode_both at (1, 128)
    int64_t r0, c0;
    int h, wd;
    if (!rowwise) {
        // transposed tile t = q nR + i, which is its place in scales_t: rows 128 i .., columns q tkw ..
        const int64_t q = t / a.nR, i = t - q * a.nR;
        r0 = kTile * i;
        c0 = q * a.tkw;
        h = (int)(a.R - r0 < kTile ? a.R - r0 : kTile);
        wd = (int)(a.K - c0 < a.tkw ? a.K - c0 : a.tkw);
    } else {
        const int64_t t2 = t - a.tiles_t, row = t2 / a.nK, j = t2 - row * a.nK;
        r0 = row;
        c0 = kTile * j;
        h = 1;
        wd = (int)(a.K - c0 < kTile ? a.K - c0 : kTile);
    }
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
    if (lane == 0) {
        if (rowwise) {
            a.scales[t - a.tiles_t] = k.x;
        } else {
            a.scales_t[t] = k.x;
            if constexpr (OP == kOpBoth && TILE == kTileFull) a.scales[(r0 >> 7) * a.nK + (c0 >> 7)] = k.x;
        }
    }
    for (int e = lane; e < n; e += 64) {
        const int i = e / wd, j = e - i * wd;
        const int64_t at = (r0 + i) * a.K + c0 + j;
        uint8_t code;
        if constexpr (SR) code = (uint8_t)code1_sr<F>(IN::load1(x + at), k, mx_draw1(a.sr, a.sr.offset + (uint64_t)at));
        else code = (uint8_t)code1<F>(IN::load1(x + at), k);
        if (rowwise) {
            a.codes[at] = code;
        } else {
            a.codes_t[(c0 + j) * a.R + r0 + i] = code;
            if constexpr (OP == kOpBoth && TILE == kTileFull) a.codes[at] = code;
        }
    }
}

// ---- host side ----
inline int tile_kind(int tr, int tk)
{
    if (tr == 1 && tk == kTile) return kTileRow;
    if (tr == kTile && tk == kTile) return kTileFull;
    return -1;                                  // (128, 1) among them: the operand of no product
}

// THE launch rule of the four launching entries: which kernel, with which hints and which store width
int ocpbt_route(int64_t R, int64_t K, int tr, int tk, int x_type, int aligned16, fp8q_ocpbt_route_info *info)
{
    if (!info || R <= 0 || K <= 0 || R > INT64_MAX / K) return FP8Q_EINVAL;
    if (tile_kind(tr, tk) < 0) return FP8Q_EUNSUPPORTED;
    if (x_type != FP8Q_DT_F32 && !half_type(x_type)) return FP8Q_EINVAL;
    const bool panel = aligned16 && K % 4 == 0;
    fp8q_ocpbt_route_info r = {};
    r.kernel = panel ? FP8Q_OCPBT_PANEL : FP8Q_OCPBT_PLAIN;
    r.code_store_bytes = !panel ? 1 : (R % 16 == 0 ? 16 : (R % 4 == 0 ? 4 : 1));
    r.nontemporal = panel && R * K >= kNtBytes / 4;
    *info = r;
    return FP8Q_OK;
}

// Argument checks (everything is reported before the launch, in ocpb_launch's order and with its codes) and the one launch.
// codes / scales: the row-wise operands of encode_both, null for encode_t.  sr: the seed and offset of a stochastic-rounding
// entry, null for round to nearest even.
template <int OP>
int ocpbt_launch(const void *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int x_type, int64_t R,
                 int64_t K, int tr, int tk, int fmt, float eps, hipStream_t st, const MxSr *sr = nullptr)
{
    if (!x || !codes_t || !scales_t || (OP == kOpBoth && (!codes || !scales)) || R <= 0 || K <= 0 || R > INT64_MAX / K)
        return FP8Q_EINVAL;
    const int kind = tile_kind(tr, tk);
    if ((fmt != FP8Q_OCP_E4M3FN && fmt != FP8Q_OCP_E5M2) || kind < 0) return FP8Q_EUNSUPPORTED;
    if (value_side_misaligned(x, x_type) || (((uintptr_t)scales | (uintptr_t)scales_t) & 3)) return FP8Q_EINVAL;
    if (sr && (sr->offset & 7u)) return FP8Q_EINVAL;
    const uintptr_t ptrs = (uintptr_t)x | (uintptr_t)codes | (uintptr_t)scales | (uintptr_t)codes_t | (uintptr_t)scales_t;
    fp8q_ocpbt_route_info route;                // (encode_t passes null for what it does not take)
    if (int rc = ocpbt_route(R, K, tr, tk, x_type, (ptrs & 15) == 0, &route)) return rc;
    const bool panel = route.kernel == FP8Q_OCPBT_PANEL;
    OcpbtSrArgs a = {};
    if (sr) a.sr = *sr;
    a.codes = codes;
    a.codes_t = codes_t;
    a.scales = scales;
    a.scales_t = scales_t;
    a.R = R;
    a.K = K;
    a.nR = cdiv(R, kTile);
    a.nK = cdiv(K, kTile);
    a.tkw = kind == kTileRow ? 1 : kTile;
    a.gran = route.code_store_bytes;
    a.eps = eps;
    int64_t grid;
    if (panel) {
        grid = a.nR > (int64_t)INT32_MAX / a.nK ? (int64_t)INT32_MAX + 1 : a.nR * a.nK;
    } else {
        // R * K fits: so do K * nR, nK * nR and R * nK, and the sum of two of them
        a.tiles_t = (kind == kTileRow ? K : a.nK) * a.nR;
        const int64_t rows = (OP == kOpBoth && kind == kTileRow) ? R * a.nK : 0;
        if (a.tiles_t > INT64_MAX - rows) return FP8Q_EINVAL;
        a.tiles = a.tiles_t + rows;
        grid = cdiv(a.tiles, kBlock / 64);
    }
    if (grid > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    const dim3 g((unsigned)grid), b(kBlock);
    value_io(x_type, [&](auto in) {
        typedef decltype(in) IN;
        dispatch<FP8Q_OCP_E4M3FN, FP8Q_OCP_E5M2>(fmt, [&](auto fc) {
            constexpr int F = decltype(fc)::value;
            dispatch<(int)kTileRow, (int)kTileFull>(kind, [&](auto tc) {
                constexpr int TILE = decltype(tc)::value;
                dispatch<true, false>(sr != nullptr, [&](auto src) {
                    constexpr bool SR = decltype(src)::value;
                    const OcpbtArgsOf<SR> &as = a;      // (the round-to-nearest-even kernels take the OcpbtArgs part)
                    if (!panel) {
                        hipLaunchKernelGGL((k_ocpbt_plain<OP, F, IN, TILE, SR>), g, b, 0, st, x, as);
                    } else {
                        dispatch<true, false>(route.nontemporal != 0, [&](auto ntc) {
                            constexpr bool NT = decltype(ntc)::value;
                            hipLaunchKernelGGL((k_ocpbt_panel<OP, F, IN, TILE, NT, SR>), g, b, 0, st, x, as);
                        });
                    }
                });
            });
        });
    });
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_ocpbt_route(int64_t R, int64_t K, int tile_r, int tile_k, int x_type, int aligned16, fp8q_ocpbt_route_info *info)
{
    return ocpbt_route(R, K, tile_r, tile_k, x_type, aligned16, info);
}

int fp8q_ocpbt_encode_f32(const float *x, uint8_t *codes_t, float *scales_t, int64_t R, int64_t K, int tile_r, int tile_k,
                          int fmt, float eps, fp8q_stream_t stream)
{
    return ocpbt_launch<kOpT>(x, nullptr, nullptr, codes_t, scales_t, FP8Q_DT_F32, R, K, tile_r, tile_k, fmt, eps,
                              (hipStream_t)stream);
}

int fp8q_ocpbt_encode_h16(const void *x, uint8_t *codes_t, float *scales_t, int x_type, int64_t R, int64_t K, int tile_r,
                          int tile_k, int fmt, float eps, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    return ocpbt_launch<kOpT>(x, nullptr, nullptr, codes_t, scales_t, x_type, R, K, tile_r, tile_k, fmt, eps,
                              (hipStream_t)stream);
}

int fp8q_ocpbt_encode_both_f32(const float *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int64_t R,
                               int64_t K, int tile_r, int tile_k, int fmt, float eps, fp8q_stream_t stream)
{
    return ocpbt_launch<kOpBoth>(x, codes, scales, codes_t, scales_t, FP8Q_DT_F32, R, K, tile_r, tile_k, fmt, eps,
                                 (hipStream_t)stream);
}

int fp8q_ocpbt_encode_both_h16(const void *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int x_type,
                               int64_t R, int64_t K, int tile_r, int tile_k, int fmt, float eps, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    return ocpbt_launch<kOpBoth>(x, codes, scales, codes_t, scales_t, x_type, R, K, tile_r, tile_k, fmt, eps,
                                 (hipStream_t)stream);
}

int fp8q_ocpbtsr_encode_f32(const float *x, uint8_t *codes_t, float *scales_t, int64_t R, int64_t K, int tile_r, int tile_k,
                            int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return ocpbt_launch<kOpT>(x, nullptr, nullptr, codes_t, scales_t, FP8Q_DT_F32, R, K, tile_r, tile_k, fmt, eps,
                              (hipStream_t)stream, &sr);
}

int fp8q_ocpbtsr_encode_h16(const void *x, uint8_t *codes_t, float *scales_t, int x_type, int64_t R, int64_t K, int tile_r,
                            int tile_k, int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    const MxSr sr = mx_sr_args(seed, offset);
    return ocpbt_launch<kOpT>(x, nullptr, nullptr, codes_t, scales_t, x_type, R, K, tile_r, tile_k, fmt, eps,
                              (hipStream_t)stream, &sr);
}

int fp8q_ocpbtsr_encode_both_f32(const float *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int64_t R,
                                 int64_t K, int tile_r, int tile_k, int fmt, float eps, uint64_t seed, uint64_t offset,
                                 fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return ocpbt_launch<kOpBoth>(x, codes, scales, codes_t, scales_t, FP8Q_DT_F32, R, K, tile_r, tile_k, fmt, eps,
                                 (hipStream_t)stream, &sr);
}

int fp8q_ocpbtsr_encode_both_h16(const void *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int x_type,
                                 int64_t R, int64_t K, int tile_r, int tile_k, int fmt, float eps, uint64_t seed,
                                 uint64_t offset, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    const MxSr sr = mx_sr_args(seed, offset);
    return ocpbt_launch<kOpBoth>(x, codes, scales, codes_t, scales_t, x_type, R, K, tile_r, tile_k, fmt, eps,
                                 (hipStream_t)stream, &sr);
}

}  // extern "C"
