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
// group is -1 (or, defensively, not in [0, G), or row0 not in [start, end)), recomputes end, and runs the tile body that
// k_mxmm runs (fp8q_mmq.h's mm_mx_tile: prologue, step loop, store) on X rows [row0, min(row0 + TM, end)) and the group's W:
// codes at wc + g * N * wpitch, scales at ws + g * N * kblocks.  (g * N * wpitch is a multiple of the pitch, so mm_load_width
// of the base pointer holds for every group.)  X rows past `end` are zero codes under scale byte 127, never the next group's
// rows; stores are masked by m < end, n < N.
// The body's geometry (TM, WM waves along M, WN waves along N):
//   TM = 128, 2 x 2: k_mxmm's geometry, 64 x 64 per wave, acc[4][4].
//   TM = 32,  1 x 4: the four waves split N.  Wave w takes all 32 rows of X and W rows [32 w, 32 w + 32): 2 x 2 instructions
//        per step into acc[2][2], 16 accumulator registers.  The W panel is unchanged; the X panel is MmPanel<bits, 32>: 256 /
//        192 / 128 chunks of 16 bytes per step (FP8 / FP6 / FP4), at most one per lane, lanes past the count idle.  LDS is at
//        most 2 x (16 + 4) KiB.  Bank arithmetic: the swizzle (FP8 / FP4) and the 112-byte pitch (FP6) are functions of the row
//        alone, a read pass is still one lane group over 16 consecutive rows from a multiple of 16, and a write pass still
//        consecutive lanes over consecutive chunks of a row, so fp8q_mx_mm.hip's header holds line for line for 32 rows.
// Each output element is the same ascending chain of instructions over the same two rows as in k_mxmm, from a zero
// accumulator: the same bits as fp8q_mxmm_nt on the group's slices, whichever TM (at TM = 128 it is the same code).
#include "fp8q_mmq.h"

namespace {

constexpr int kGmMaxGroups = 4096;
constexpr int kGmMaxTiles = 65535;                      // grid.y

struct GmPlan {
    int64_t tile_m, m_tiles_max, ws_bytes;
};

struct GmArgs : MxOperands {            // X: the rows of all groups; W: rows g * N + n
    const void *offsets;                // [G + 1], int64 (off64) or int32
    const int2 *table;                  // [m_tiles_max] of (group, row0), k_mxg_map's
    int64_t T;
    int G, off64;
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

template <int FX, int FW, int TM, int WM, int WN>
__global__ void __launch_bounds__(kMmBlock)
k_mxgmm(const GmArgs a)
{
    const int2 entry = a.table[blockIdx.y];
    const int grp = entry.x;
    if (grp < 0 || grp >= a.G) return;
    int64_t start, end;
    gm_group_rows(a.offsets, a.off64, grp, a.T, start, end);
    const int64_t m0 = entry.y;
    if (m0 < start || m0 >= end) return;
    mm_mx_tile<FX, FW, TM, WM, WN>(a, m0, (int64_t)blockIdx.x * kMmTile, end, a.wc + (int64_t)grp * a.N * a.wpitch,
                                   a.ws + (int64_t)grp * a.N * a.kblocks);
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
    const int ybytes = mm_y_bytes(y_type);
    if (!ybytes) return FP8Q_EINVAL;
    if (T == 0 || N == 0 || G == 0) return FP8Q_OK;
    if (!xc || !xs || !wc || !ws || !offsets || !y) return FP8Q_EINVAL;
    if ((uintptr_t)y % (uintptr_t)ybytes || (uintptr_t)offsets % (uintptr_t)(off64 ? 8 : 4)) return FP8Q_EINVAL;
    if (!workspace || workspace_bytes < p.ws_bytes || (uintptr_t)workspace % 16) return FP8Q_EINVAL;
    const int64_t kblocks = K / 32, gn = cdiv(N, kMmTile);
    // G * N * wpitch and T * N are byte and element offsets in int64: G <= 2^12, pitch <= 32 kblocks
    if (kblocks > (int64_t)INT32_MAX || gn > (int64_t)INT32_MAX || N > (INT64_MAX >> 13) / (32 * kblocks) || T > INT64_MAX / N)
        return FP8Q_EINVAL;
    GmArgs a;
    mm_mx_operands(a, xc, xs, wc, ws, K, x_fmt, w_fmt);
    a.y = y, a.N = N;
    a.y_type = y_type;
    a.vec_store = mm_vec_store(N, y, ybytes);
    a.offsets = offsets, a.table = static_cast<const int2 *>(workspace);
    a.T = T, a.G = (int)G, a.off64 = off64;
    hipLaunchKernelGGL(k_mxg_map, dim3(1), dim3(kMmBlock), 0, st, offsets, off64, (int)G, T, (int)p.tile_m,
                       static_cast<int2 *>(workspace), (int)p.m_tiles_max);
    if (const int rc = launch_rc()) return rc;
    const dim3 grid((unsigned)gn, (unsigned)p.m_tiles_max), block(kMmBlock);
    mm_dispatch_mx_pair(x_fmt, w_fmt, [&](auto FX, auto FW) {
        if (p.tile_m == 32) hipLaunchKernelGGL((k_mxgmm<FX(), FW(), 32, 1, 4>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_mxgmm<FX(), FW(), 128, 2, 2>), grid, block, 0, st, a);
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
