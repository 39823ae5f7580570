// fp8q_mmq.h -- what the five matrix-core products share.  fp8q_mx_mm.hip's header has the instruction's operand and result
// layouts and the LDS bank arithmetic.  Internal linkage, as fp8q_common.h.
//   The tile: 128 rows of either operand under 256 lanes, MmPanel (one K step of an operand in LDS), mm_load_chunk (a 16-byte
//     chunk by loads that narrow with the operand's alignment), mm_load_panel / mm_store_panel, mm_read_frag (what a lane hands
//     to the matrix instruction), mm_store4 and mm_store_tile (the masked stores of a wave's results).
//     Users: k_mxmm, k_mxgmm, k_ocpbmm, k_i8mm (which walks its tile itself, around its per-element correction); k_mxsk takes
//     mm_load_chunk and mm_store4 alone, k_mxsk_reduce mm_store4.
//   The MX products (fp8q_mx_mm.hip, its small-M kernel fp8q_mx_mm_skinny.hip, its grouped form fp8q_mx_mm_grouped.hip): the
//     format table MmFmt, the operand block MxOperands that their kernels' arguments start with, mm_load_scales, and
//     mm_mx_tile, the one tile body -- prologue, step loop, store -- that k_mxmm and k_mxgmm are.  k_mxsk has its own loop.
//   Host side: mm_y_bytes and mm_vec_store (all five launchers), mm_load_width (the one rule for the load width),
//     mm_tile_grid (the grid of 128 x 128 tiles and what it refuses), and for the MX launchers mm_fmt_known, mm_block_bytes,
//     mm_mx_operands (fills the block) and mm_dispatch_mx_pair.
// The double-buffered K-step loop stands three times: in mm_mx_tile, in k_ocpbmm (fp8q_ocp_block_mm.hip, with its float32
// scales) and in k_i8mm (fp8q_int_mm.hip).  One skeleton with a policy per product gave the same bits and was measured:
// the grouped product's 32-row kernels ran 5 to 7 % slower and the OCP product 1 to 7 %, with equal registers, LDS and
// occupancy -- the compiler lays the loop out anew at every touch (profiles/mm_pipeline_ab.txt; k_i8mm's store through
// mm_store_tile with an element map cost it about 1.5 % in the same way).  Whoever changes the loop changes it three times
// until that is solved.
#pragma once
#include "fp8q_half.h"

namespace {

constexpr int kMmTile = 128;     // rows of either operand under one workgroup
constexpr int kMmBlock = 256;

typedef int i8v __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));

// ---- the MX formats ----
constexpr int kMmScaleOne = 127; // the E8M0 byte of 2^0: what masked rows and blocks carry

// FP8Q_MX_* -> the instruction's format number and the element width
template <int F> struct MmFmt;
template <> struct MmFmt<FP8Q_MX_E4M3FN> { static constexpr int hw = 0, bits = 8; };
template <> struct MmFmt<FP8Q_MX_E5M2> { static constexpr int hw = 1, bits = 8; };
template <> struct MmFmt<FP8Q_MX_E2M3> { static constexpr int hw = 2, bits = 6; };
template <> struct MmFmt<FP8Q_MX_E3M2> { static constexpr int hw = 3, bits = 6; };
template <> struct MmFmt<FP8Q_MX_E2M1> { static constexpr int hw = 4, bits = 4; };

// one operand's panel of a K step in LDS (fp8q_mx_mm.hip's header has the bank arithmetic).  ROWS is 128 everywhere but in
// fp8q_mx_mm_grouped.hip's 32-row X panel, whose 256 / 192 / 128 chunks leave lanes idle (kWhole false): chunk_at depends on
// the row alone, so the layout and its bank arithmetic hold for any multiple of 16 rows.
template <int BITS, int ROWS = kMmTile>
struct MmPanel {
    static constexpr int kBlockBytes = 4 * BITS;            // one MX block: 32 / 24 / 16
    static constexpr int kStepBytes = 4 * kBlockBytes;      // a row's four blocks: 128 / 96 / 64
    static constexpr int kChunks = kStepBytes / 16;         // 8 / 6 / 4
    static constexpr bool kSwizzle = BITS != 6;
    static constexpr int kPitch = kSwizzle ? kStepBytes : kStepBytes + 16;
    static constexpr int kBytes = ROWS * kPitch;
    static constexpr int kCount = ROWS * kChunks;                           // the panel's chunks
    static constexpr int kPerLane = (kCount + kMmBlock - 1) / kMmBlock;     // 128 rows: 4 / 3 / 2 chunks per lane
    static constexpr bool kWhole = kCount % kMmBlock == 0;                  // every lane has kPerLane chunks
    static __device__ __forceinline__ int chunk_at(int row, int c)
    {
        if constexpr (kSwizzle) return row * kPitch + 16 * (c ^ ((row / (256 / kStepBytes)) % kChunks));
        else return row * kPitch + 16 * c;
    }
};

// the first `nvalid` bytes at p, zero-extended to 16, by loads of w bytes; p is w-aligned and nvalid a multiple of w (the MX
// product asks for 0, 8 or 16)
__device__ __forceinline__ u4v mm_load_chunk(const uint8_t *p, int nvalid, int w)
{
    u4v v = {0u, 0u, 0u, 0u};
    if (nvalid == 0) return v;
    if (w == 16 && nvalid == 16) return *reinterpret_cast<const u4v *>(p);
    if (w >= 8) {
        const u2v lo = *reinterpret_cast<const u2v *>(p);
        v.x = lo.x;
        v.y = lo.y;
        if (nvalid == 16) {
            const u2v hi = *reinterpret_cast<const u2v *>(p + 8);
            v.z = hi.x;
            v.w = hi.y;
        }
        return v;
    }
    uint32_t d[4] = {0u, 0u, 0u, 0u};
    if (w == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * i < nvalid) d[i] = *reinterpret_cast<const uint32_t *>(p + 4 * i);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i < nvalid) d[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
    v.x = d[0];
    v.y = d[1];
    v.z = d[2];
    v.w = d[3];
    return v;
}

// step ks of the panel rows [row0, row0 + P's rows) of an operand whose rows end at `rows`: lane tid takes the chunks tid,
// tid + 256, ... (a 32-row panel leaves lanes idle).  Chunk (r, c) is the bytes [o, o + 16) of row row0 + r, o = ks * kStepBytes
// + 16 c.  It is read only for row0 + r < rows, and then the bytes of it that lie in the row: an MX row (pitch % 8 == 0,
// o % 16 == 0) has 16, 8 or none; BYTE_TAIL, the OCP product's rows of pitch K, clamp(pitch - o, 0, 16), a multiple of w
// because w divides K.  Every byte read lies in [row * pitch, row * pitch + pitch) of a buffer of rows * pitch bytes.
template <class P, bool BYTE_TAIL = false>
__device__ __forceinline__ void mm_load_panel(u4v (&g)[P::kPerLane], const uint8_t *codes, int64_t pitch, int64_t rows,
                                              int64_t row0, int ks, int w, int tid)
{
#pragma unroll
    for (int j = 0; j < P::kPerLane; ++j) {
        const int q = tid + j * kMmBlock, r = q / P::kChunks, c = q % P::kChunks;
        const int64_t row = row0 + r, o = (int64_t)ks * P::kStepBytes + 16 * c, left = pitch - o;
        const bool in = (P::kWhole || q < P::kCount) && row < rows;
        const int tail = BYTE_TAIL ? (left > 0 ? (int)left : 0) : (left >= 8 ? 8 : 0);
        g[j] = mm_load_chunk(codes + row * pitch + o, in ? (left >= 16 ? 16 : tail) : 0, w);
    }
}

template <class P>
__device__ __forceinline__ void mm_store_panel(uint8_t *s, const u4v (&g)[P::kPerLane], int tid)
{
#pragma unroll
    for (int j = 0; j < P::kPerLane; ++j) {
        const int q = tid + j * kMmBlock;
        if (!P::kWhole && q >= P::kCount) continue;
        *reinterpret_cast<u4v *>(s + P::chunk_at(q / P::kChunks, q % P::kChunks)) = g[j];
    }
}

// a lane's operand of panel row `row` (FP6 / FP4: block g; FP8: the two 16-byte runs of fp8q_mx_mm.hip's header), the registers
// past the format's 8 / 6 / 4 unused by the instruction
template <class P>
__device__ __forceinline__ i8v mm_read_frag(const uint8_t *s, int row, int g)
{
    i8v f = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (P::kBlockBytes == 32) {
        const u4v lo = *reinterpret_cast<const u4v *>(s + P::chunk_at(row, g));          // K [16 g, 16 g + 16) of the step
        const u4v hi = *reinterpret_cast<const u4v *>(s + P::chunk_at(row, 4 + g));      // K [64 + 16 g, 64 + 16 g + 16)
        f[0] = (int)lo.x, f[1] = (int)lo.y, f[2] = (int)lo.z, f[3] = (int)lo.w;
        f[4] = (int)hi.x, f[5] = (int)hi.y, f[6] = (int)hi.z, f[7] = (int)hi.w;
    } else if constexpr (P::kBlockBytes == 16) {
        const u4v lo = *reinterpret_cast<const u4v *>(s + P::chunk_at(row, g));
        f[0] = (int)lo.x, f[1] = (int)lo.y, f[2] = (int)lo.z, f[3] = (int)lo.w;
    } else {
        const u2v *p = reinterpret_cast<const u2v *>(s + row * P::kPitch + 24 * g);
        const u2v a = p[0], b = p[1], c = p[2];
        f[0] = (int)a.x, f[1] = (int)a.y, f[2] = (int)b.x, f[3] = (int)b.y, f[4] = (int)c.x, f[5] = (int)c.y;
    }
    return f;
}

// y[e .. e + 3] (the first `n` of them) = v, a half type rounded once; vec: one store of the four
template <class T>
__device__ __forceinline__ void mm_store4_half(uint16_t *y, int64_t e, const f4v v, int n, bool vec)
{
    if (vec) {
        u2v h;
        h.x = T::narrow2(v[0], v[1]);
        h.y = T::narrow2(v[2], v[3]);
        *reinterpret_cast<u2v *>(y + e) = h;
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < n) y[e + r] = T::narrow1(v[r]);
}

__device__ __forceinline__ void mm_store4(void *y, int y_type, int64_t e, const f4v v, int n, bool vec)
{
    if (y_type == FP8Q_DT_F16) return mm_store4_half<F16>(static_cast<uint16_t *>(y), e, v, n, vec);
    if (y_type == FP8Q_DT_BF16) return mm_store4_half<BF16>(static_cast<uint16_t *>(y), e, v, n, vec);
    float *yf = static_cast<float *>(y);
    if (vec) {
        *reinterpret_cast<f4v *>(yf + e) = v;
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < n) yf[e + r] = v[r];
}

// a wave's IW x JX results: lane l, register r of acc[i][j] is y[m + 16 j][n + 16 i + r], m and n the lane's first row and
// column (row l % 16 of the wave's first X fragment, column 4 (l / 16) of its first W fragment); masked by m_end and N
template <int IW, int JX>
__device__ __forceinline__ void mm_store_tile(const f4v (&acc)[IW][JX], void *y, int y_type, int64_t N, int64_t m, int64_t m_end,
                                              int64_t n, bool vec)
{
#pragma unroll
    for (int j = 0; j < JX; ++j) {
        const int64_t mj = m + 16 * j;
        if (mj >= m_end) continue;
#pragma unroll
        for (int i = 0; i < IW; ++i) {
            const int64_t ni = n + 16 * i;
            if (ni >= N) continue;
            const int64_t left = N - ni;
            mm_store4(y, y_type, mj * N + ni, acc[i][j], left < 4 ? (int)left : 4, vec);
        }
    }
}

// ---- the MX products' operand block and tile body ----
// what the kernels of the three MX products take first; each adds its own (MmArgs, SkArgs, GmArgs)
struct MxOperands {
    const uint8_t *xc, *xs, *wc, *ws;   // codes and scales of X (rows m) and W (rows n)
    void *y;
    int64_t N, kblocks;                 // kblocks = K / 32
    int64_t xpitch, wpitch;             // bytes of a codes row
    int nsteps;                         // ceil(K / 128)
    int xw, ww;                         // bytes per global load of either operand's codes: 16, 8, 4 or 1
    int y_type;                         // FP8Q_DT_* of what the launch stores
    int vec_store;                      // N % 4 == 0 and y aligned to four of its elements
};

// the scale bytes of block `blk` of the rows row, row + 16, ...; 127 where the row or the block does not exist
template <int NF>
__device__ __forceinline__ void mm_load_scales(int (&s)[NF], const uint8_t *scales, int64_t rows, int64_t row, int64_t blk,
                                               int64_t kblocks)
{
#pragma unroll
    for (int t = 0; t < NF; ++t) {
        const int64_t r = row + 16 * t;
        s[t] = (r < rows && blk < kblocks) ? (int)scales[r * kblocks + blk] : kMmScaleOne;
    }
}

// One workgroup's tile of an MX product: y[m0 .. min(m0 + TM, m_end))[n0 .. min(n0 + 128, N)) = X . W^T with W's codes and
// scales at wc / ws (a.wc / a.ws, or a group's).  fp8q_mx_mm.hip's header has the loop and the LDS layout.  The four waves are
// WM along M x WN along N; a wave owns TM / WM rows of X (JX fragments of 16) and 128 / WN rows of W (IW fragments), IW x JX
// instructions per step into acc[IW][JX].  X rows from m_end on are zero codes under scale byte 127 and are not stored.
// Every lane of the workgroup calls it or none does: it holds the step loop's barriers.  A kernel calls it once: the panels are
// its __shared__ arrays.
template <int FX, int FW, int TM, int WM, int WN>
__device__ __forceinline__ void mm_mx_tile(const MxOperands &a, int64_t m0, int64_t n0, int64_t m_end, const uint8_t *wc,
                                           const uint8_t *ws)
{
    static_assert(WM * WN == 4 && TM % (16 * WM) == 0 && kMmTile % (16 * WN) == 0, "four waves tile TM x 128");
    using PX = MmPanel<MmFmt<FX>::bits, TM>;
    using PW = MmPanel<MmFmt<FW>::bits>;
    constexpr int XR = TM / WM, WR = kMmTile / WN;      // the wave's rows of X and of W
    constexpr int JX = XR / 16, IW = WR / 16;
    __shared__ __attribute__((aligned(16))) uint8_t s_x[2][PX::kBytes];
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][PW::kBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lr = lane & 15, lg = lane >> 4;       // the lane's row of an instruction; the MX block of the step it scales
    const int64_t xrow = m0 + wm * XR + lr, wrow = n0 + wn * WR + lr;   // (+ 16 j / 16 i: the rows whose scales the lane feeds)

    u4v gx[PX::kPerLane], gw[PW::kPerLane];
    int sx[JX], sw[IW], sx_next[JX], sw_next[IW];
    f4v acc[IW][JX];    // [i: W's 16 rows][j: X's 16 rows]
#pragma unroll
    for (int i = 0; i < IW; ++i)
#pragma unroll
        for (int j = 0; j < JX; ++j) acc[i][j] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

    mm_load_panel<PX>(gx, a.xc, a.xpitch, m_end, m0, 0, a.xw, tid);
    mm_load_panel<PW>(gw, wc, a.wpitch, a.N, n0, 0, a.ww, tid);
    mm_load_scales<JX>(sx, a.xs, m_end, xrow, lg, a.kblocks);
    mm_load_scales<IW>(sw, ws, a.N, wrow, lg, a.kblocks);
    mm_store_panel<PX>(s_x[0], gx, tid);
    mm_store_panel<PW>(s_w[0], gw, tid);
    __syncthreads();

    for (int ks = 0; ks < a.nsteps; ++ks) {
        const int buf = ks & 1;
        const bool more = ks + 1 < a.nsteps;
        if (more) {         // the next step's loads fly over this step's instructions
            mm_load_panel<PX>(gx, a.xc, a.xpitch, m_end, m0, ks + 1, a.xw, tid);
            mm_load_panel<PW>(gw, wc, a.wpitch, a.N, n0, ks + 1, a.ww, tid);
            mm_load_scales<JX>(sx_next, a.xs, m_end, xrow, 4 * (int64_t)(ks + 1) + lg, a.kblocks);
            mm_load_scales<IW>(sw_next, ws, a.N, wrow, 4 * (int64_t)(ks + 1) + lg, a.kblocks);
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
    mm_store_tile<IW, JX>(acc, a.y, a.y_type, a.N, xrow, m_end, n0 + wn * WR + 4 * lg, a.vec_store != 0);
}

// ---- host side ----
// the five MX element formats and the bytes of one block of 32 elements
inline bool mm_fmt_known(int f)
{
    return f == FP8Q_MX_E4M3FN || f == FP8Q_MX_E5M2 || f == FP8Q_MX_E2M1 || f == FP8Q_MX_E2M3 || f == FP8Q_MX_E3M2;
}

inline int mm_block_bytes(int f) { return f == FP8Q_MX_E2M1 ? 16 : ((f == FP8Q_MX_E2M3 || f == FP8Q_MX_E3M2) ? 24 : 32); }

// The one place that decides how a codes operand is loaded: the widest of 16, 8, 4 bytes that divides both the pointer and the
// row pitch (so that every row, and every 16-byte chunk of it, starts aligned), else single bytes.
inline int mm_load_width(const void *codes, int64_t pitch)
{
    for (int w = 16; w >= 4; w >>= 1)
        if ((uintptr_t)codes % (uintptr_t)w == 0 && pitch % w == 0) return w;
    return 1;
}

// bytes of one element of y; 0 for a type that no product stores
inline int mm_y_bytes(int y_type) { return y_type == FP8Q_DT_F32 ? 4 : (half_type(y_type) ? 2 : 0); }

// one store of a lane's four results: N % 4 == 0 and y aligned to four of its elements
inline int mm_vec_store(int64_t N, const void *y, int ybytes) { return N % 4 == 0 && (uintptr_t)y % (uintptr_t)(4 * ybytes) == 0; }

// the grid of 128 x 128 tiles over y[M, N] (M, N >= 1), gn x gm with N fastest; false where grid.y, grid.x or an element index
// of y in int64 cannot hold it
inline bool mm_tile_grid(int64_t M, int64_t N, int64_t &gm, int64_t &gn)
{
    gm = cdiv(M, kMmTile), gn = cdiv(N, kMmTile);
    return gm <= 65535 && gn <= (int64_t)INT32_MAX && M <= INT64_MAX / N;
}

// the operands' part of an MX launch (K % 32 == 0 and K / 32 <= INT32_MAX checked by the caller); y, N, y_type and vec_store
// are the launcher's.  w6: the widest load of an FP6 operand, 16 where chunks start 16-aligned (the panels), 8 where a lane's
// fragment starts at a multiple of 24 bytes (the skinny kernel).
inline void mm_mx_operands(MxOperands &a, const uint8_t *xc, const uint8_t *xs, const uint8_t *wc, const uint8_t *ws, int64_t K,
                           int x_fmt, int w_fmt, int w6 = 16)
{
    a.xc = xc, a.xs = xs, a.wc = wc, a.ws = ws;
    a.kblocks = K / 32;
    a.xpitch = a.kblocks * mm_block_bytes(x_fmt);
    a.wpitch = a.kblocks * mm_block_bytes(w_fmt);
    a.nsteps = (int)cdiv(a.kblocks, 4);
    a.xw = std::min(mm_load_width(xc, a.xpitch), mm_block_bytes(x_fmt) == 24 ? w6 : 16);
    a.ww = std::min(mm_load_width(wc, a.wpitch), mm_block_bytes(w_fmt) == 24 ? w6 : 16);
}

// f(FX, FW) with both formats as constants: the 25 pairs
template <class F>
inline void mm_dispatch_mx_pair(int x_fmt, int w_fmt, F &&f)
{
    dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M1, FP8Q_MX_E2M3, FP8Q_MX_E3M2>(x_fmt, [&](auto FX) {
        dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M1, FP8Q_MX_E2M3, FP8Q_MX_E3M2>(w_fmt, [&](auto FW) { f(FX, FW); });
    });
}

}  // namespace
