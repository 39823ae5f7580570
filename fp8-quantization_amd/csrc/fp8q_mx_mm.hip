// fp8q_mx_mm.hip -- the product of two MX operands on gfx950's matrix cores: y[M, N] = A[M, K] . B[N, K]^T, both operands K
// contiguous and block-scaled exactly as fp8q_mx.hip / fp8q_mx_t.hip write them (codes in 32 / 24 / 16 bytes per block of 32,
// one E8M0 byte per block in plain [rows, K / 32] order).  include/fp8q.h states the contract: the product of the operands'
// decoded values, accumulated in float32 by v_mfma_scale_f32_16x16x128_f8f6f4 in an order the instruction does not specify.
// K % 32 == 0; short last blocks and batched B are out of scope; split-K for M <= 64 is fp8q_mx_mm_skinny.hip's kernel.
//
// The instruction.  One v_mfma_scale_f32_16x16x128_f8f6f4 multiplies 16 rows x 128 K of its "A" operand with 16 rows x 128 K
// of its "B" operand.  Lane l holds, of either operand, row l % 16, g = l / 16.  FP6 and FP4: the K elements [32 g, 32 g + 32),
// ONE MX block, 24 / 16 consecutive bytes of a codes row in 6 / 4 VGPRs.  FP8, 8 VGPRs: registers 0-3 are the 16 elements
// [16 g, 16 g + 16) and registers 4-7 the 16 elements [64 + 16 g, 64 + 16 g + 16) -- two 16-byte runs 64 bytes apart, halves of
// the blocks g / 2 and 2 + g / 2 (tests/test_mx_mm_gpu.py's exact cases are what establishes this: with 32 consecutive bytes
// in the lane, registers 4-7 were multiplied under the scale of lane group 2).  Either way the bytes are straight copies of
// what the encoders wrote.  The scale operand is one VGPR whose byte 0 is, in every format, the E8M0 byte of block g of the
// lane's row -- the block [32 g, 32 g + 32) of the step, whichever lanes hold its elements.  The result: lane l, register r holds
// D[4 g + r][l % 16], the first index the "A" operand's row.  So the function's B (the weights, rows n) is the instruction's A
// and the function's A (the activations, rows m) its B: a lane's four registers are y[m][n .. n + 3], one 16-byte store
// (8 bytes of a half type) with no transposition.  Below, X is the function's A and W the function's B.  cbsz is W's format
// number, blgp X's (E4M3 0, E5M2 1, E2M3 2, E3M2 3, E2M1 4), template constants.
//
// k_mxmm<FX, FW>: a workgroup of 256 lanes = 4 waves takes a tile of 128 (M) x 128 (N), grid ceil(N / 128) x ceil(M / 128);
// wave w the 64 x 64 quarter (w / 2, w % 2): 4 x 4 instructions per K step of 128 elements (four MX blocks), 64 accumulator
// registers.  Per step the 128-row panels of both operands (128 / 96 / 64 bytes a row) go global -> registers -> LDS in 16-byte
// chunks, consecutive lanes taking consecutive chunks of a row; there are two LDS buffers, the next step's global loads are
// issued before this step's instructions and written to the other buffer after them, one barrier per step.  A chunk is loaded
// with the widest loads that the operand's pointer and row pitch allow (16, 8, 4 or 1 bytes: mm_load_width, a uniform kernel
// argument; FP8 / FP4 pitches are multiples of 16, an FP6 pitch of 24 K / 32 bytes only of 8).  Scale bytes are not staged: a
// lane reads the 4 + 4 single bytes of its rows' blocks from global together with the panel, one step ahead (the dword a
// K % 128 == 0 row would allow carries three bytes the lane has no use for).
// Edges: a chunk is read only where it lies wholly inside its row -- rows past M / N and the K tail (K % 128 != 0: 1-3 valid
// blocks in the last step) are zero codes under the scale byte 127, never a load past a row's end and never the next row's
// bytes; an FP6 chunk that straddles the end of its row (pitch % 16 == 8) loads its first 8 bytes.  Stores are masked by m < M,
// n < N; an N % 4 != 0 (or a y off its 16- / 8-byte alignment) takes scalar stores.
// LDS layout, by the rule bank = (byte address / 4) mod 64, a 16-lane group (one g, the 16 rows of an instruction) per pass:
//   FP8  pitch 128 bytes, unpadded (two operands x two buffers are exactly 64 KiB); chunk c of row r lies at chunk
//        c ^ ((r / 2) % 8).  Lane (r, g) reads chunks g and 4 + g; for one of them the 16 rows start at dword
//        32 (r % 2) + 4 (c ^ ((r / 2) % 8)): sixteen different multiples of 4, four banks each -- all 64 banks once.
//   FP4  pitch 64 bytes, chunk c at c ^ ((r / 4) % 4): dword 16 (r % 4) + 4 (c ^ ((r / 4) % 4)), again sixteen different ones.
//   FP6  a lane's 24 bytes are three 8-byte reads and do not fit a 16-byte swizzle: pitch 96 + 16 = 112 bytes = 28 dwords, and
//        28 r mod 64 over r = 0 .. 15 is sixteen different multiples of 4 (0 28 56 20 48 12 40 4 32 60 24 52 16 44 8 36), two
//        banks per read: conflict-free.
//   Writes are one 16-byte chunk per lane, consecutive lanes consecutive chunks of a row: 8 (FP8) or 4 (FP4) lanes fill one
//   row's banks under a permutation, the next row the other half (FP8) or the next quarter (FP4): conflict-free per 16 lanes.
// There is no float arithmetic outside the instruction and the final conversion to a half type.
// The tile, the panel, the chunk load, the fragment read, the stores and mm_load_width are in fp8q_mmq.h, which
// fp8q_ocp_block_mm.hip shares; the MX format table (MmFmt, mm_fmt_known, mm_block_bytes) is there too, shared with the
// small-M kernel of fp8q_mx_mm_skinny.hip.
#include "fp8q_mmq.h"

namespace {

struct MmArgs {
    const uint8_t *xc, *xs, *wc, *ws;   // codes and scales of X (rows m) and W (rows n)
    void *y;
    int64_t M, N, kblocks;              // kblocks = K / 32
    int64_t xpitch, wpitch;             // bytes of a codes row
    int nsteps;                         // ceil(K / 128)
    int xw, ww;                         // bytes per global load of either operand's codes: 16, 8, 4 or 1
    int y_type;                         // FP8Q_DT_*
    int vec_store;                      // N % 4 == 0 and y aligned to four of its elements
};

// step ks of the panel rows [row0, row0 + 128): lane tid takes the chunks tid, tid + 256, ...  Chunk (r, c) is the bytes
// [o, o + 16) of row row0 + r, o = ks * kStepBytes + 16 c.  It is read only for row0 + r < rows, and then its first
// min(pitch - o, 16) bytes where that is positive: pitch % 8 == 0 and o % 16 == 0, so this is 16, 8 or nothing, and every
// byte read lies in [row * pitch, row * pitch + pitch) of a buffer of rows * pitch bytes.
template <class P>
__device__ __forceinline__ void mm_load_panel(u4v (&g)[P::kPerLane], const uint8_t *codes, int64_t pitch, int64_t rows,
                                              int64_t row0, int ks, int w, int tid)
{
#pragma unroll
    for (int j = 0; j < P::kPerLane; ++j) {
        const int q = tid + j * kMmBlock, r = q / P::kChunks, c = q % P::kChunks;
        const int64_t row = row0 + r, o = (int64_t)ks * P::kStepBytes + 16 * c, left = pitch - o;
        const int nvalid = row < rows ? (left >= 16 ? 16 : (left >= 8 ? 8 : 0)) : 0;
        g[j] = mm_load_chunk(codes + row * pitch + o, nvalid, w);
    }
}

// the scale bytes of block `blk` of the rows row, row + 16, row + 32, row + 48; 127 where the row or the block does not exist
__device__ __forceinline__ void mm_load_scales(int (&s)[4], const uint8_t *scales, int64_t rows, int64_t row, int64_t blk,
                                               int64_t kblocks)
{
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t r = row + 16 * t;
        s[t] = (r < rows && blk < kblocks) ? (int)scales[r * kblocks + blk] : kMmScaleOne;
    }
}

template <int FX, int FW>
__global__ void __launch_bounds__(kMmBlock)
k_mxmm(const MmArgs a)
{
    using PX = MmPanel<MmFmt<FX>::bits>;
    using PW = MmPanel<MmFmt<FW>::bits>;
    __shared__ __attribute__((aligned(16))) uint8_t s_x[2][PX::kBytes];
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][PW::kBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;        // the wave's 64 x 64 quarter
    const int lr = lane & 15, lg = lane >> 4;       // the lane's row of an instruction; the MX block of the step it scales
    const int64_t m0 = (int64_t)blockIdx.y * kMmTile, n0 = (int64_t)blockIdx.x * kMmTile;
    const int64_t xrow = m0 + wm * 64 + lr, wrow = n0 + wn * 64 + lr;   // (+ 16 j / 16 i: the rows whose scales the lane feeds)

    u4v gx[PX::kPerLane], gw[PW::kPerLane];
    int sx[4], sw[4], sx_next[4], sw_next[4];
    f4v acc[4][4];      // [i: W's 16 rows][j: X's 16 rows]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

    mm_load_panel<PX>(gx, a.xc, a.xpitch, a.M, m0, 0, a.xw, tid);
    mm_load_panel<PW>(gw, a.wc, a.wpitch, a.N, n0, 0, a.ww, tid);
    mm_load_scales(sx, a.xs, a.M, xrow, lg, a.kblocks);
    mm_load_scales(sw, a.ws, a.N, wrow, lg, a.kblocks);
    mm_store_panel<PX>(s_x[0], gx, tid);
    mm_store_panel<PW>(s_w[0], gw, tid);
    __syncthreads();

    for (int ks = 0; ks < a.nsteps; ++ks) {
        const int buf = ks & 1;
        const bool more = ks + 1 < a.nsteps;
        if (more) {         // the next step's loads fly over this step's instructions
            mm_load_panel<PX>(gx, a.xc, a.xpitch, a.M, m0, ks + 1, a.xw, tid);
            mm_load_panel<PW>(gw, a.wc, a.wpitch, a.N, n0, ks + 1, a.ww, tid);
            mm_load_scales(sx_next, a.xs, a.M, xrow, 4 * (int64_t)(ks + 1) + lg, a.kblocks);
            mm_load_scales(sw_next, a.ws, a.N, wrow, 4 * (int64_t)(ks + 1) + lg, a.kblocks);
        }
        i8v fw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fw[i] = mm_read_frag<PW>(s_w[buf], wn * 64 + 16 * i + lr, lg);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i8v fx = mm_read_frag<PX>(s_x[buf], wm * 64 + 16 * j + lr, lg);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[i], fx, acc[i][j], MmFmt<FW>::hw, MmFmt<FX>::hw,
                                                                             0, sw[i], 0, sx[j]);
        }
        if (more) {
            // the other buffer: every wave left it at the barrier that ended the step before
            mm_store_panel<PX>(s_x[buf ^ 1], gx, tid);
            mm_store_panel<PW>(s_w[buf ^ 1], gw, tid);
#pragma unroll
            for (int t = 0; t < 4; ++t) sx[t] = sx_next[t], sw[t] = sw_next[t];
        }
        __syncthreads();
    }

    // lane l, register r of acc[i][j]: y[m0 + 64 wm + 16 j + l % 16][n0 + 64 wn + 16 i + 4 (l / 16) + r]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t m = xrow + 16 * j;
        if (m >= a.M) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t n = n0 + wn * 64 + 16 * i + 4 * lg;
            if (n >= a.N) continue;
            const int64_t left = a.N - n;
            mm_store4(a.y, a.y_type, m * a.N + n, acc[i][j], left < 4 ? (int)left : 4, a.vec_store != 0);
        }
    }
}

// ---- host side ----
int mm_launch(const uint8_t *xc, const uint8_t *xs, const uint8_t *wc, const uint8_t *ws, void *y, int64_t M, int64_t N,
              int64_t K, int x_fmt, int w_fmt, int y_type, hipStream_t st)
{
    if (!mm_fmt_known(x_fmt) || !mm_fmt_known(w_fmt)) return FP8Q_EUNSUPPORTED;
    if (K <= 0 || K % 32 || M < 0 || N < 0) return FP8Q_EINVAL;
    if (y_type != FP8Q_DT_F32 && !half_type(y_type)) return FP8Q_EINVAL;
    if (M == 0 || N == 0) return FP8Q_OK;
    if (!xc || !xs || !wc || !ws || !y) return FP8Q_EINVAL;
    const int ybytes = y_type == FP8Q_DT_F32 ? 4 : 2;
    if ((uintptr_t)y % (uintptr_t)ybytes) return FP8Q_EINVAL;
    const int64_t kblocks = K / 32, gm = cdiv(M, kMmTile), gn = cdiv(N, kMmTile);
    if (kblocks > (int64_t)INT32_MAX || gm > 65535 || gn > (int64_t)INT32_MAX || M > INT64_MAX / N) return FP8Q_EINVAL;
    MmArgs a;
    a.xc = xc, a.xs = xs, a.wc = wc, a.ws = ws, a.y = y;
    a.M = M, a.N = N, a.kblocks = kblocks;
    a.xpitch = kblocks * mm_block_bytes(x_fmt);
    a.wpitch = kblocks * mm_block_bytes(w_fmt);
    a.nsteps = (int)cdiv(kblocks, 4);
    a.xw = mm_load_width(xc, a.xpitch);
    a.ww = mm_load_width(wc, a.wpitch);
    a.y_type = y_type;
    a.vec_store = N % 4 == 0 && (uintptr_t)y % (uintptr_t)(4 * ybytes) == 0;
    const dim3 grid((unsigned)gn, (unsigned)gm), block(kMmBlock);
    dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M1, FP8Q_MX_E2M3, FP8Q_MX_E3M2>(x_fmt, [&](auto FX) {
        dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M1, FP8Q_MX_E2M3, FP8Q_MX_E3M2>(w_fmt, [&](auto FW) {
            hipLaunchKernelGGL((k_mxmm<FX(), FW()>), grid, block, 0, st, a);
        });
    });
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_mxmm_nt(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *b_codes, const uint8_t *b_scales, void *y,
                 int64_t M, int64_t N, int64_t K, int a_fmt, int b_fmt, int y_type, fp8q_stream_t stream)
{
    return mm_launch(a_codes, a_scales, b_codes, b_scales, y, M, N, K, a_fmt, b_fmt, y_type, (hipStream_t)stream);
}

}  // extern "C"
