// fp8q_mx_mm_grouped.hip -- the grouped MX product: y[o_g : o_{g+1}, :] = A[o_g : o_{g+1}, :] . B[g]^T for every group g of a
// mixture-of-experts layer, A's T rows sorted by group, B [G, N, K] one MX weight matrix per group, `offsets` [G + 1] a device
// tensor that only the kernels read: two launches and no host decision that depends on its contents.  Operands, formats,
// K % 32 == 0 and the instruction are those of fp8q_mx_mm.hip, whose header states the lane and result layouts and the LDS
// bank arithmetic; X is the function's A, W its B, W the instruction's "A".  include/fp8q.h states the contract and the plan.
//
// The clamp.  For group g: start = min(max(o_g, 0), T), end = min(max(o_{g+1}, start), T).  It is local to the group (no prefix
// maximum), both kernels compute it from offsets[g] and offsets[g + 1] alone, and 0 <= start <= end <= T whatever the
// offsets hold: every X row read and every y row written lies in [start, end), so offsets outside the contract give
// unspecified values in y (groups may overlap, rows may be written twice or not at all), never an access outside the operands.
//
// k_mxg_map: one workgroup of 256 lanes turns offsets into workspace[m_tiles_max] of (int32 group, int32 row0), the M tiles of
// all groups in ascending group, ascending row order.  Lane l owns the ceil(G / 256) <= 16 consecutive groups from
// l * ceil(G / 256): it loads their offsets (independent loads, no chain), forms tiles_g = ceil((end - start) / TM) and their
// running sum in int64 (out-of-contract offsets can make the total exceed 2^31), the 256 lane totals are scanned in LDS
// (Hillis-Steele, 8 rounds), and pref[g], the exclusive prefix sum, lands in LDS (4097 x 8 bytes).  Then lane l fills entries
// t = l, l + 256, ... < m_tiles_max: an upper-bound binary search of pref for the one group with pref[g] <= t < pref[g + 1]
// (empty groups share their successor's prefix and are skipped by it), row0 = start_g + (t - pref[g]) * TM; entries from
// pref[G] on get group -1.  Entries at index >= m_tiles_max do not exist and are never written: in-contract offsets never
// need them (the plan's m_tiles_max is the maximum over all count vectors), out-of-contract ones lose those tiles.
//
// k_mxgmm<FX, FW, TM, WM, WN>: grid ceil(N / 128) x m_tiles_max, N fastest as in k_mxmm, so the workgroups that share an X
// tile and the ones that share a group's W panel run together.  A workgroup loads its table entry (8 bytes), returns if the
// group is -1 (or, defensively, not in [0, G), or row0 not in [start, end)), recomputes end, and runs k_mxmm's step loop --
// two LDS buffers, the next step's global loads issued before this step's instructions, one barrier per step -- on X rows
// [row0, min(row0 + TM, end)) and the group's W: codes at wc + g * N * wpitch, scales at ws + g * N * kblocks.  (g * N * wpitch
// is a multiple of the pitch, so mm_load_width of the base pointer holds for every group.)  X rows past `end` are zero codes
// under scale byte 127, never the next group's rows; stores are masked by m < end, n < N.
// One body over (TM, WM waves along M, WN waves along N), WM * WN = 4; a wave owns TM / WM rows of X (JX fragments of 16) and
// 128 / WN rows of W (IW fragments), IW x JX instructions per step into acc[IW][JX]:
//   TM = 128, 2 x 2: k_mxmm's geometry, 64 x 64 per wave, acc[4][4].
//   TM = 32,  1 x 4: the four waves split N.  Wave w takes all 32 rows of X and W rows [32 w, 32 w + 32): 2 x 2 instructions
//        per step into acc[2][2], 16 accumulator registers.  The W panel is unchanged; the X panel is MmPanel<bits, 32>: 256 /
//        192 / 128 chunks of 16 bytes per step (FP8 / FP6 / FP4), at most one per lane, lanes past the count idle.  LDS is at
//        most 2 x (16 + 4) KiB.  Bank arithmetic: the swizzle (FP8 / FP4) and the 112-byte pitch (FP6) are functions of the row
//        alone, a read pass is still one lane group over 16 consecutive rows from a multiple of 16, and a write pass still
//        consecutive lanes over consecutive chunks of a row, so fp8q_mx_mm.hip's header holds line for line for 32 rows.
// Each output element is the same ascending chain of instructions over the same two rows as in k_mxmm, from a zero
// accumulator: the same bits as fp8q_mxmm_nt on the group's slices, whichever TM.
#include "fp8q_mmq.h"

namespace {

constexpr int kGmMaxGroups = 4096;
constexpr int kGmMaxTiles = 65535;                      // grid.y

struct GmPlan {
    int64_t tile_m, m_tiles_max, ws_bytes;
};

struct GmArgs {
    const uint8_t *xc, *xs, *wc, *ws;   // codes and scales of X (rows m, all groups) and W (rows g * N + n)
    void *y;
    const void *offsets;                // [G + 1], int64 (off64) or int32
    const int2 *table;                  // [m_tiles_max] of (group, row0), k_mxg_map's
    int64_t T, N, kblocks;              // kblocks = K / 32
    int64_t xpitch, wpitch;             // bytes of a codes row
    int G, off64;
    int nsteps;                         // ceil(K / 128)
    int xw, ww;                         // bytes per global load of either operand's codes: 16, 8, 4 or 1
    int y_type;                         // FP8Q_DT_*
    int vec_store;                      // N % 4 == 0 and y aligned to four of its elements
};

// rows [start, end) of group g, 0 <= start <= end <= T whatever offsets[g], offsets[g + 1] hold (the header's clamp)
__device__ __forceinline__ void gm_group_rows(const void *offsets, int off64, int g, int64_t T, int64_t &start, int64_t &end)
{
    int64_t o0, o1;
    if (off64) o0 = static_cast<const int64_t *>(offsets)[g], o1 = static_cast<const int64_t *>(offsets)[g + 1];
    else o0 = static_cast<const int32_t *>(offsets)[g], o1 = static_cast<const int32_t *>(offsets)[g + 1];
    start = o0 < 0 ? 0 : (o0 > T ? T : o0);
    end = o1 < start ? start : (o1 > T ? T : o1);
}

__global__ void __launch_bounds__(kMmBlock)
k_mxg_map(const void *offsets, int off64, int G, int64_t T, int TM, int2 *table, int m_tiles_max)
{
    __shared__ int64_t s_pref[kGmMaxGroups + 1];
    __shared__ int64_t s_tot[kMmBlock];
    const int tid = threadIdx.x, per = (G + kMmBlock - 1) / kMmBlock, g0 = tid * per;
    int64_t run = 0;
#pragma unroll 4
    for (int i = 0; i < per; ++i) {
        const int g = g0 + i;
        if (g >= G) break;
        int64_t start, end;
        gm_group_rows(offsets, off64, g, T, start, end);
        s_pref[g] = run;
        run += (end - start + TM - 1) / TM;
    }
    s_tot[tid] = run;
    __syncthreads();
    for (int d = 1; d < kMmBlock; d <<= 1) {
        const int64_t add = tid >= d ? s_tot[tid - d] : 0;
        __syncthreads();
        s_tot[tid] += add;
        __syncthreads();
    }
    const int64_t base = s_tot[tid] - run;      // the lanes before this one
    for (int i = 0; i < per; ++i) {
        const int g = g0 + i;
        if (g >= G) break;
        s_pref[g] += base;
    }
    if (tid == kMmBlock - 1) s_pref[G] = s_tot[tid];
    __syncthreads();
    const int64_t total = s_pref[G];
    for (int t = tid; t < m_tiles_max; t += kMmBlock) {
        int2 e = make_int2(-1, 0);
        if (t < total) {
            int lo = 1, hi = G;     // the first i in [1, G] with pref[i] > t; pref[0] = 0 <= t < pref[G]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_pref[mid] > t) hi = mid;
                else lo = mid + 1;
            }
            const int g = lo - 1;
            int64_t start, end;
            gm_group_rows(offsets, off64, g, T, start, end);
            e.x = g;
            e.y = (int)(start + (t - s_pref[g]) * TM);      // < end <= T <= INT32_MAX
        }
        table[t] = e;
    }
}

// step ks of the panel rows [row0, row0 + P's rows) of an operand whose rows end at `rows`: fp8q_mx_mm.hip's mm_load_panel (a
// chunk is read only for a row < rows and only where it lies in its row: 16, 8 or no bytes), with the lanes past a 32-row
// panel's chunk count idle
template <class P>
__device__ __forceinline__ void gm_load_panel(u4v (&g)[P::kPerLane], const uint8_t *codes, int64_t pitch, int64_t rows,
                                              int64_t row0, int ks, int w, int tid)
{
#pragma unroll
    for (int j = 0; j < P::kPerLane; ++j) {
        const int q = tid + j * kMmBlock, r = q / P::kChunks, c = q % P::kChunks;
        const int64_t row = row0 + r, o = (int64_t)ks * P::kStepBytes + 16 * c, left = pitch - o;
        const bool in = (P::kWhole || q < P::kCount) && row < rows;
        const int nvalid = in ? (left >= 16 ? 16 : (left >= 8 ? 8 : 0)) : 0;
        g[j] = mm_load_chunk(codes + row * pitch + o, nvalid, w);
    }
}

// the scale bytes of block `blk` of the rows row, row + 16, ...; 127 where the row or the block does not exist
template <int NF>
__device__ __forceinline__ void gm_load_scales(int (&s)[NF], const uint8_t *scales, int64_t rows, int64_t row, int64_t blk,
                                               int64_t kblocks)
{
#pragma unroll
    for (int t = 0; t < NF; ++t) {
        const int64_t r = row + 16 * t;
        s[t] = (r < rows && blk < kblocks) ? (int)scales[r * kblocks + blk] : kMmScaleOne;
    }
}

template <int FX, int FW, int TM, int WM, int WN>
__global__ void __launch_bounds__(kMmBlock)
k_mxgmm(const GmArgs a)
{
    static_assert(WM * WN == 4 && TM % (16 * WM) == 0 && kMmTile % (16 * WN) == 0, "four waves tile TM x 128");
    using PX = MmPanel<MmFmt<FX>::bits, TM>;
    using PW = MmPanel<MmFmt<FW>::bits>;
    constexpr int XR = TM / WM, WR = kMmTile / WN;      // the wave's rows of X and of W
    constexpr int JX = XR / 16, IW = WR / 16;
    __shared__ __attribute__((aligned(16))) uint8_t s_x[2][PX::kBytes];
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][PW::kBytes];

    const int2 entry = a.table[blockIdx.y];
    const int grp = entry.x;
    if (grp < 0 || grp >= a.G) return;
    int64_t start, end;
    gm_group_rows(a.offsets, a.off64, grp, a.T, start, end);
    const int64_t m0 = entry.y;
    if (m0 < start || m0 >= end) return;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lr = lane & 15, lg = lane >> 4;       // the lane's row of an instruction; the MX block of the step it scales
    const int64_t n0 = (int64_t)blockIdx.x * kMmTile;
    const int64_t xrow = m0 + wm * XR + lr, wrow = n0 + wn * WR + lr;   // (+ 16 j / 16 i: the rows whose scales the lane feeds)
    const uint8_t *wc = a.wc + (int64_t)grp * a.N * a.wpitch, *ws = a.ws + (int64_t)grp * a.N * a.kblocks;

    u4v gx[PX::kPerLane], gw[PW::kPerLane];
    int sx[JX], sw[IW], sx_next[JX], sw_next[IW];
    f4v acc[IW][JX];    // [i: W's 16 rows][j: X's 16 rows]
#pragma unroll
    for (int i = 0; i < IW; ++i)
#pragma unroll
        for (int j = 0; j < JX; ++j) acc[i][j] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

    gm_load_panel<PX>(gx, a.xc, a.xpitch, end, m0, 0, a.xw, tid);
    gm_load_panel<PW>(gw, wc, a.wpitch, a.N, n0, 0, a.ww, tid);
    gm_load_scales<JX>(sx, a.xs, end, xrow, lg, a.kblocks);
    gm_load_scales<IW>(sw, ws, a.N, wrow, lg, a.kblocks);
    mm_store_panel<PX>(s_x[0], gx, tid);
    mm_store_panel<PW>(s_w[0], gw, tid);
    __syncthreads();

    for (int ks = 0; ks < a.nsteps; ++ks) {
        const int buf = ks & 1;
        const bool more = ks + 1 < a.nsteps;
        if (more) {         // the next step's loads fly over this step's instructions
            gm_load_panel<PX>(gx, a.xc, a.xpitch, end, m0, ks + 1, a.xw, tid);
            gm_load_panel<PW>(gw, wc, a.wpitch, a.N, n0, ks + 1, a.ww, tid);
            gm_load_scales<JX>(sx_next, a.xs, end, xrow, 4 * (int64_t)(ks + 1) + lg, a.kblocks);
            gm_load_scales<IW>(sw_next, ws, a.N, wrow, 4 * (int64_t)(ks + 1) + lg, a.kblocks);
        }
        i8v fw[IW];
#pragma unroll
        for (int i = 0; i < IW; ++i) fw[i] = mm_read_frag<PW>(s_w[buf], wn * WR + 16 * i + lr, lg);
#pragma unroll
        for (int j = 0; j < JX; ++j) {
            const i8v fx = mm_read_frag<PX>(s_x[buf], wm * XR + 16 * j + lr, lg);
#pragma unroll
            for (int i = 0; i < IW; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[i], fx, acc[i][j], MmFmt<FW>::hw, MmFmt<FX>::hw,
                                                                             0, sw[i], 0, sx[j]);
        }
        if (more) {
            // the other buffer: every wave left it at the barrier that ended the step before
            mm_store_panel<PX>(s_x[buf ^ 1], gx, tid);
            mm_store_panel<PW>(s_w[buf ^ 1], gw, tid);
#pragma unroll
            for (int t = 0; t < JX; ++t) sx[t] = sx_next[t];
#pragma unroll
            for (int t = 0; t < IW; ++t) sw[t] = sw_next[t];
        }
        __syncthreads();
    }

    // lane l, register r of acc[i][j]: y[m0 + XR wm + 16 j + l % 16][n0 + WR wn + 16 i + 4 (l / 16) + r]
#pragma unroll
    for (int j = 0; j < JX; ++j) {
        const int64_t m = xrow + 16 * j;
        if (m >= end) continue;
#pragma unroll
        for (int i = 0; i < IW; ++i) {
            const int64_t n = n0 + wn * WR + 16 * i + 4 * lg;
            if (n >= a.N) continue;
            const int64_t left = a.N - n;
            mm_store4(a.y, a.y_type, m * a.N + n, acc[i][j], left < 4 ? (int)left : 4, a.vec_store != 0);
        }
    }
}

// ---- host side ----
// The one place that decides the tile height and the table's length (include/fp8q.h states the rule).  tile_m_req 0: the
// plan chooses.
int gm_plan(int64_t T, int64_t N, int64_t K, int64_t G, int64_t tile_m_req, GmPlan &p)
{
    if (G > kGmMaxGroups || (tile_m_req != 0 && tile_m_req != 32 && tile_m_req != 128)) return FP8Q_EUNSUPPORTED;
    if (K <= 0 || K % 32 || T < 0 || N < 0 || G < 0 || T > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    const int64_t n = std::min(G, T);
    p.tile_m = tile_m_req ? tile_m_req : (T <= 32 * n ? 32 : 128);
    p.m_tiles_max = n ? (T - n) / p.tile_m + n : 0;     // no group, no tile: the formula's n - 1 one-row groups need n >= 1
    if (p.m_tiles_max > kGmMaxTiles) return FP8Q_EINVAL;
    p.ws_bytes = 8 * p.m_tiles_max;
    return FP8Q_OK;
}

int gm_launch(const uint8_t *xc, const uint8_t *xs, const uint8_t *wc, const uint8_t *ws, const void *offsets, int off64,
              void *y, int64_t T, int64_t N, int64_t K, int64_t G, int x_fmt, int w_fmt, int y_type, int64_t tile_m_req,
              void *workspace, int64_t workspace_bytes, hipStream_t st)
{
    if (!mm_fmt_known(x_fmt) || !mm_fmt_known(w_fmt)) return FP8Q_EUNSUPPORTED;
    GmPlan p;
    if (const int rc = gm_plan(T, N, K, G, tile_m_req, p)) return rc;
    if (y_type != FP8Q_DT_F32 && !half_type(y_type)) return FP8Q_EINVAL;
    if (T == 0 || N == 0 || G == 0) return FP8Q_OK;
    if (!xc || !xs || !wc || !ws || !offsets || !y) return FP8Q_EINVAL;
    const int ybytes = y_type == FP8Q_DT_F32 ? 4 : 2;
    if ((uintptr_t)y % (uintptr_t)ybytes || (uintptr_t)offsets % (uintptr_t)(off64 ? 8 : 4)) return FP8Q_EINVAL;
    if (!workspace || workspace_bytes < p.ws_bytes || (uintptr_t)workspace % 16) return FP8Q_EINVAL;
    const int64_t kblocks = K / 32, gn = cdiv(N, kMmTile);
    // G * N * wpitch and T * N are byte and element offsets in int64: G <= 2^12, pitch <= 32 kblocks
    if (kblocks > (int64_t)INT32_MAX || gn > (int64_t)INT32_MAX || N > (INT64_MAX >> 13) / (32 * kblocks) || T > INT64_MAX / N)
        return FP8Q_EINVAL;
    GmArgs a;
    a.xc = xc, a.xs = xs, a.wc = wc, a.ws = ws, a.y = y;
    a.offsets = offsets, a.table = static_cast<const int2 *>(workspace);
    a.T = T, a.N = N, a.kblocks = kblocks;
    a.xpitch = kblocks * mm_block_bytes(x_fmt);
    a.wpitch = kblocks * mm_block_bytes(w_fmt);
    a.G = (int)G, a.off64 = off64;
    a.nsteps = (int)cdiv(kblocks, 4);
    a.xw = mm_load_width(xc, a.xpitch);
    a.ww = mm_load_width(wc, a.wpitch);
    a.y_type = y_type;
    a.vec_store = N % 4 == 0 && (uintptr_t)y % (uintptr_t)(4 * ybytes) == 0;
    hipLaunchKernelGGL(k_mxg_map, dim3(1), dim3(kMmBlock), 0, st, offsets, off64, (int)G, T, (int)p.tile_m,
                       static_cast<int2 *>(workspace), (int)p.m_tiles_max);
    if (const int rc = launch_rc()) return rc;
    const dim3 grid((unsigned)gn, (unsigned)p.m_tiles_max), block(kMmBlock);
    dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M1, FP8Q_MX_E2M3, FP8Q_MX_E3M2>(x_fmt, [&](auto FX) {
        dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M1, FP8Q_MX_E2M3, FP8Q_MX_E3M2>(w_fmt, [&](auto FW) {
            if (p.tile_m == 32) hipLaunchKernelGGL((k_mxgmm<FX(), FW(), 32, 1, 4>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_mxgmm<FX(), FW(), 128, 2, 2>), grid, block, 0, st, a);
        });
    });
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_mxgmm_plan(int64_t T, int64_t N, int64_t K, int64_t G, int64_t tile_m_req, int64_t *plan3)
{
    GmPlan p;
    if (!plan3) return FP8Q_EINVAL;
    if (const int rc = gm_plan(T, N, K, G, tile_m_req, p)) return rc;
    plan3[0] = p.tile_m, plan3[1] = p.m_tiles_max, plan3[2] = p.ws_bytes;
    return FP8Q_OK;
}

int fp8q_mxgmm_nt(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *b_codes, const uint8_t *b_scales,
                  const void *offsets, int offsets_64, void *y, int64_t T, int64_t N, int64_t K, int64_t G, int a_fmt, int b_fmt,
                  int y_type, int64_t tile_m_req, void *workspace, int64_t workspace_bytes, fp8q_stream_t stream)
{
    return gm_launch(a_codes, a_scales, b_codes, b_scales, offsets, offsets_64, y, T, N, K, G, a_fmt, b_fmt, y_type, tile_m_req,
                     workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
