// fp8q_ocp_block_mm.hip -- the product of two block-scaled hardware FP8 operands on gfx950's matrix cores:
// y[M, N] = A[M, K] . B[N, K]^T, both operands K contiguous exactly as fp8q_ocp_block.hip / fp8q_ocp_block_t.hip write them
// (E4M3FN / E5M2 codes [rows, K], a float32 scale per 1x128 or 128x128 tile, [ceil(rows / tile_r), ceil(K / 128)] row-major).
// include/fp8q.h states the contract:  y[m, n] = sum over K tiles t, ascending, of (sa[ra(m), t] * sb[rb(n), t]) * P_t[m, n].
//
// Float32 scales cannot go into the instruction as E8M0 bytes can (fp8q_mx_mm.hip), and a K tile of 128 is exactly one
// v_mfma_f32_16x16x128_f8f6f4 deep.  So every instruction starts from a ZERO accumulator and leaves the tile's partial product
// P_t unscaled in temporaries; the vector ALU promotes it into the float32 accumulator, acc = fma(P_t, sa * sb, acc), one fused
// operation per result and step, sa * sb one float32 multiplication.  The instruction is the builtin
// __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4 with both scale operands the constant 0, which the compiler selects as the
// unscaled v_mfma_f32_16x16x128_f8f6f4 (no scale operand is encoded); the exact GPU tests show that it multiplies by 1.
//
// Geometry (fp8q_mx_mm.hip's, whose header has the operand, result and LDS layouts; the shared pieces are in fp8q_mmq.h).  A
// workgroup of 256 lanes = 4 waves takes a tile of 128 (M) x 128 (N), grid ceil(N / 128) x ceil(M / 128); wave w the 64 x 64
// quarter (w / 2, w % 2), 4 x 4 instructions per K step of 128.  Below X is the function's A (rows m) and W the function's B
// (rows n); W is the instruction's A operand, so lane l, register r of acc[i][j] is y[m][n + r] with m = 64 wm + 16 j + l % 16
// and n = 64 wn + 16 i + 4 (l / 16).  The FP8 panels go global -> registers -> LDS in 16-byte chunks under the pitch-128 XOR
// swizzle, two buffers, the next step's loads issued before this step's instructions, one barrier per step.
//
// The inner loop.  A step's 16 instructions are written as four groups of four (one X fragment j against the four W fragments),
// each group into one of two sets of 16 temporaries, a group's promotion behind the NEXT group's instructions.  The compiler
// does not keep that order: in the emitted loop all 16 matrix instructions of a step come first (4, the X fragment reads, 12,
// the LDS writes of the next panels), then the 1 to 64 scale products and the 64 fused multiply-adds, then the barrier; 64
// temporaries are live.  So a wave's promotion follows its own matrix work and overlaps only with the matrix work of the other
// wave on its SIMD.  That is why the kernels ask for two workgroups per CU: unbounded, the 1x128 x 1x128 ones took 201 VGPRs +
// 64 AGPRs and ran one wave per SIMD; bounded, all 16 stay under 256 registers with no scratch
// (profiles/ocpb_mm_resources.txt), and two workgroups' 2 x 66 KiB of LDS fit a CU's 160 KiB.  A
// __builtin_amdgcn_sched_barrier between the groups left the emitted order as it was; enforcing it is the open end.  Per lane
// and step: 64 fused multiply-adds, and 4 scale products when W carries 128x128 tiles (sw is then one value for the workgroup
// and the product depends on j alone), 64 when it carries 1x128 tiles (the four registers of a result are four rows n).
//
// Scales.  A 128x128 tile is exactly one workgroup row / column: its scale for a step is ONE address for every lane, loaded one
// step ahead (XT / WT = true).  The 128 row scales of a 1x128 operand lie a scale row (4 ceil(K / 128) bytes) apart: lanes
// 0-127 fetch X's and lanes 128-255 W's, one each, one step ahead with the panels, and put them into a double-buffered
// float[2][128] per operand beside the panels (1 KiB each on top of the 64 KiB of panels); after the step's barrier a lane reads
// its 4 X scales and, as four 16-byte reads, its 16 W scales.  No column-strided load is repeated per lane.
//
// Edges.  Codes of rows past M / N and of K past the end are zero codes and are never read: a chunk's valid bytes are
// clamp(K - offset, 0, 16), which is a multiple of the load width because the width divides K, so no load passes its row's end
// or touches the next row.  Row scales past M / N are 0.0f.  Every scale tile t < ceil(K / 128) exists, so a short last tile
// multiplies its zero tail under its own scale.  With finite scales no NaN can arise from the masked part (0 * finite), and
// masked rows are not stored.  The load width (16, 8, 4 or 1 bytes) is mm_load_width's: pointer and K.
#include "fp8q_mmq.h"

namespace {

using ObPanel = MmPanel<8>;

struct ObArgs {
    const uint8_t *xc, *wc;     // codes of X (rows m) and W (rows n), pitch K
    const float *xs, *ws;       // their scales, pitch nsteps
    void *y;
    int64_t M, N, K;
    int nsteps;                 // ceil(K / 128): the K tiles, and the pitch of both scale arrays
    int xw, ww;                 // bytes per global load of either operand's codes: 16, 8, 4 or 1
    int y_type;                 // FP8Q_DT_*
    int vec_store;              // N % 4 == 0 and y aligned to four of its elements
};

// What a lane fetches of step ks's scales, one step ahead.  TILED: the one scale of the workgroup's 128x128 tile (row0 / 128 is
// its scale row; row0 < rows, so it exists).  Otherwise the scale of row row0 + slot, lanes 0-127 (slot = tid) for X and
// 128-255 (slot = tid - 128) for W, 0.0f past the operand's rows; the other lanes fetch nothing.
template <bool TILED>
__device__ __forceinline__ float ob_fetch_scale(const float *scales, int64_t rows, int64_t row0, int slot, int nsteps, int ks)
{
    if constexpr (TILED) return scales[(row0 / kMmTile) * nsteps + ks];
    const int64_t row = row0 + slot;
    return (slot >= 0 && slot < kMmTile && row < rows) ? scales[row * nsteps + ks] : 0.0f;
}

template <int FX, int FW, bool XT, bool WT>
__global__ void __launch_bounds__(kMmBlock, 2)
k_ocpbmm(const ObArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_x[2][ObPanel::kBytes];
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][ObPanel::kBytes];
    __shared__ __attribute__((aligned(16))) float s_sx[2][kMmTile];
    __shared__ __attribute__((aligned(16))) float s_sw[2][kMmTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;        // the wave's 64 x 64 quarter
    const int lr = lane & 15, lg = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.y * kMmTile, n0 = (int64_t)blockIdx.x * kMmTile;
    const int xslot = tid, wslot = tid - kMmTile;

    u4v gx[ObPanel::kPerLane], gw[ObPanel::kPerLane];
    f4v acc[4][4];      // [i: W's 16 rows][j: X's 16 rows]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

    mm_load_panel<ObPanel, true>(gx, a.xc, a.K, a.M, m0, 0, a.xw, tid);
    mm_load_panel<ObPanel, true>(gw, a.wc, a.K, a.N, n0, 0, a.ww, tid);
    float ux = ob_fetch_scale<XT>(a.xs, a.M, m0, xslot, a.nsteps, 0);      // TILED: the step's scale; else in flight to LDS
    float uw = ob_fetch_scale<WT>(a.ws, a.N, n0, wslot, a.nsteps, 0);
    mm_store_panel<ObPanel>(s_x[0], gx, tid);
    mm_store_panel<ObPanel>(s_w[0], gw, tid);
    if (!XT && xslot < kMmTile) s_sx[0][xslot] = ux;
    if (!WT && wslot >= 0) s_sw[0][wslot] = uw;
    __syncthreads();

    for (int ks = 0; ks < a.nsteps; ++ks) {
        const int buf = ks & 1;
        const bool more = ks + 1 < a.nsteps;
        float ux_next = 0.0f, uw_next = 0.0f;
        if (more) {         // the next step's loads fly over this step's instructions
            mm_load_panel<ObPanel, true>(gx, a.xc, a.K, a.M, m0, ks + 1, a.xw, tid);
            mm_load_panel<ObPanel, true>(gw, a.wc, a.K, a.N, n0, ks + 1, a.ww, tid);
            ux_next = ob_fetch_scale<XT>(a.xs, a.M, m0, xslot, a.nsteps, ks + 1);
            uw_next = ob_fetch_scale<WT>(a.ws, a.N, n0, wslot, a.nsteps, ks + 1);
        }
        // this step's scales: sx[j] of the row m of group j, sw[i][r] of the row n of register r of acc[i][.]
        float sx[4];
        f4v sw[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            sx[t] = XT ? ux : s_sx[buf][wm * 64 + 16 * t + lr];
            if constexpr (!WT) sw[t] = *reinterpret_cast<const f4v *>(&s_sw[buf][wn * 64 + 16 * t + 4 * lg]);
        }
        i8v fw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fw[i] = mm_read_frag<ObPanel>(s_w[buf], wn * 64 + 16 * i + lr, lg);

        f4v p[2][4];        // two sets of temporaries as written; the compiler keeps all four groups' live
        const f4v zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j <= 4; ++j) {
            if (j < 4) {    // group j: four instructions from a zero C
                const i8v fx = mm_read_frag<ObPanel>(s_x[buf], wm * 64 + 16 * j + lr, lg);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    p[j & 1][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[i], fx, zero, FW, FX, 0, 0, 0, 0);
            }
            if (j > 0) {    // group j - 1 is folded (the compiler moves all of this behind the step's last instruction)
                const int jp = j - 1;
                const float sj = WT ? sx[jp] * uw : 0.0f;       // (W tiled: one product serves the group)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float s = WT ? sj : sx[jp] * sw[i][r];
                        acc[i][jp][r] = __builtin_fmaf(p[jp & 1][i][r], s, acc[i][jp][r]);
                    }
            }
        }
        if (more) {
            // the other buffer: every wave left it at the barrier that ended the step before
            mm_store_panel<ObPanel>(s_x[buf ^ 1], gx, tid);
            mm_store_panel<ObPanel>(s_w[buf ^ 1], gw, tid);
            if (!XT && xslot < kMmTile) s_sx[buf ^ 1][xslot] = ux_next;
            if (!WT && wslot >= 0) s_sw[buf ^ 1][wslot] = uw_next;
            ux = ux_next, uw = uw_next;
        }
        __syncthreads();
    }

    mm_store_tile<4, 4>(acc, a.y, a.y_type, a.N, m0 + wm * 64 + lr, a.M, n0 + wn * 64 + 4 * lg, a.vec_store != 0);
}

// ---- host side ----
inline bool ob_fmt_known(int f) { return f == FP8Q_OCP_E4M3FN || f == FP8Q_OCP_E5M2; }

// (1, 128) -> 1, (128, 128) -> 128, anything else (128x1 included: the operand of no product) -> 0
inline int ob_tile_rows(int tr, int tk) { return tk == kMmTile && (tr == 1 || tr == kMmTile) ? tr : 0; }

int ob_launch(const uint8_t *xc, const float *xs, const uint8_t *wc, const float *ws, void *y, int64_t M, int64_t N, int64_t K,
              int x_tr, int x_tk, int w_tr, int w_tk, int x_fmt, int w_fmt, int y_type, hipStream_t st)
{
    if (!ob_fmt_known(x_fmt) || !ob_fmt_known(w_fmt)) return FP8Q_EUNSUPPORTED;
    const int xr = ob_tile_rows(x_tr, x_tk), wr = ob_tile_rows(w_tr, w_tk);
    if (!xr || !wr) return FP8Q_EUNSUPPORTED;
    if (K <= 0 || M < 0 || N < 0) return FP8Q_EINVAL;
    const int ybytes = mm_y_bytes(y_type);
    if (!ybytes) return FP8Q_EINVAL;
    if (M == 0 || N == 0) return FP8Q_OK;
    if (!xc || !xs || !wc || !ws || !y) return FP8Q_EINVAL;
    if ((uintptr_t)y % (uintptr_t)ybytes || (uintptr_t)xs % 4 || (uintptr_t)ws % 4) return FP8Q_EINVAL;
    const int64_t nsteps = cdiv(K, kMmTile);
    int64_t gm, gn;
    if (nsteps > (int64_t)INT32_MAX || !mm_tile_grid(M, N, gm, gn) || M > INT64_MAX / K || N > INT64_MAX / K) return FP8Q_EINVAL;
    ObArgs a;
    a.xc = xc, a.wc = wc, a.xs = xs, a.ws = ws, a.y = y;
    a.M = M, a.N = N, a.K = K;
    a.nsteps = (int)nsteps;
    a.xw = mm_load_width(xc, K);
    a.ww = mm_load_width(wc, K);
    a.y_type = y_type;
    a.vec_store = mm_vec_store(N, y, ybytes);
    const dim3 grid((unsigned)gn, (unsigned)gm), block(kMmBlock);
    dispatch<FP8Q_OCP_E4M3FN, FP8Q_OCP_E5M2>(x_fmt, [&](auto FX) {
        dispatch<FP8Q_OCP_E4M3FN, FP8Q_OCP_E5M2>(w_fmt, [&](auto FW) {
            dispatch<false, true>(xr == kMmTile, [&](auto XT) {
                dispatch<false, true>(wr == kMmTile, [&](auto WT) {
                    hipLaunchKernelGGL((k_ocpbmm<FX(), FW(), XT(), WT()>), grid, block, 0, st, a);
                });
            });
        });
    });
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_ocpbmm_nt(const uint8_t *a_codes, const float *a_scales, const uint8_t *b_codes, const float *b_scales, void *y,
                   int64_t M, int64_t N, int64_t K, int a_tile_r, int a_tile_k, int b_tile_r, int b_tile_k, int a_fmt, int b_fmt,
                   int y_type, fp8q_stream_t stream)
{
    return ob_launch(a_codes, a_scales, b_codes, b_scales, y, M, N, K, a_tile_r, a_tile_k, b_tile_r, b_tile_k, a_fmt, b_fmt,
                     y_type, (hipStream_t)stream);
}

}  // extern "C"
