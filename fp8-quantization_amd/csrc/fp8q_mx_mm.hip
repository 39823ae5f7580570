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
// fp8q_mmq.h has all of it: the tile, the panel and its loaders, the fragment read, the stores, and the tile body mm_mx_tile
// that this kernel and the grouped product's (fp8q_mx_mm_grouped.hip) both are; this unit is the kernel's shell and its launcher.
#include "fp8q_mmq.h"

namespace {

struct MmArgs : MxOperands {
    int64_t M;
};

template <int FX, int FW>
__global__ void __launch_bounds__(kMmBlock)
k_mxmm(const MmArgs a)
{
    mm_mx_tile<FX, FW, kMmTile, 2, 2>(a, (int64_t)blockIdx.y * kMmTile, (int64_t)blockIdx.x * kMmTile, a.M, a.wc, a.ws);
}

// ---- host side ----
int mm_launch(const uint8_t *xc, const uint8_t *xs, const uint8_t *wc, const uint8_t *ws, void *y, int64_t M, int64_t N,
              int64_t K, int x_fmt, int w_fmt, int y_type, hipStream_t st)
{
    if (!mm_fmt_known(x_fmt) || !mm_fmt_known(w_fmt)) return FP8Q_EUNSUPPORTED;
    if (K <= 0 || K % 32 || M < 0 || N < 0) return FP8Q_EINVAL;
    const int ybytes = mm_y_bytes(y_type);
    if (!ybytes) return FP8Q_EINVAL;
    if (M == 0 || N == 0) return FP8Q_OK;
    if (!xc || !xs || !wc || !ws || !y) return FP8Q_EINVAL;
    if ((uintptr_t)y % (uintptr_t)ybytes) return FP8Q_EINVAL;
    int64_t gm, gn;
    if (K / 32 > (int64_t)INT32_MAX || !mm_tile_grid(M, N, gm, gn)) return FP8Q_EINVAL;
    MmArgs a;
    mm_mx_operands(a, xc, xs, wc, ws, K, x_fmt, w_fmt);
    a.y = y, a.M = M, a.N = N;
    a.y_type = y_type;
    a.vec_store = mm_vec_store(N, y, ybytes);
    const dim3 grid((unsigned)gn, (unsigned)gm), block(kMmBlock);
    mm_dispatch_mx_pair(x_fmt, w_fmt, [&](auto FX, auto FW) { hipLaunchKernelGGL((k_mxmm<FX(), FW()>), grid, block, 0, st, a); });
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
