// fp8q_int_mm.hip -- the product of two operands of the uniform (INT) lane's one-byte codes on gfx950's matrix cores:
// y[M, N] = A[M, K] . B[N, K]^T, both operands K contiguous exactly as fp8q_int_encode writes them for n_bits <= 8.
// include/fp8q.h states the contract:  T[m, n] = sum_k (qa[m, k] - za[m]) * (qb[n, k] - zb[n]) as an exact integer, then
// y[m, n] = fl32(fl32(T) * fl32(sa[m] * sb[n])).
//
// Geometry (fp8q_mx_mm.hip's, whose header has the LDS layout; the shared pieces are in fp8q_mmq.h as they stand).  A
// workgroup of 256 lanes = 4 waves takes a tile of 128 (M) x 128 (N), grid ceil(N / 128) x ceil(M / 128); wave w the 64 x 64
// quarter (w / 2, w % 2).  Below X is the function's A (rows m) and W the function's B (rows n).  A K step is 128 bytes of a
// row: MmPanel<8> under its XOR swizzle, global -> registers -> LDS in 16-byte chunks (mm_load_panel with the byte tail, so K
// is arbitrary and codes may sit at any address), two buffers, the next step's loads issued before this step's instructions,
// one barrier per step.
//
// The instruction is v_mfma_i32_16x16x64_i8: lane l hands it 16 bytes of row l % 16, K [16 (l / 16), 16 (l / 16) + 16) of
// its 64, for either operand, and gets the int32 results C[4 (l / 16) + r][l % 16], r < 4, rows counted in the A operand.
// W's rows are the A operand, so lane l, register r of acc[i][j] is T[m][n + r], m = 64 wm + 16 j + l % 16,
// n = 64 wn + 16 i + 4 (l / 16): mm_store4 serves unchanged.  mm_read_frag's two 16-byte runs of a row, K [16 g, 16 g + 16) and
// K [64 + 16 g, 64 + 16 g + 16) of the step, are the operands of TWO instructions per fragment pair: 32 per wave and step into
// int32 acc[4][4].  Both operands go through the same reads, so the K order is the same on both sides whatever it is; an
// integer sum does not depend on it, and the exact tests prove the row and lane mapping, not the byte order.
//
// One kernel for signed and unsigned codes.  The instruction is signed.  An operand of unsigned codes is FLIPPED:
// q' = q ^ 0x80 = q - 128 with z' = z - 128, so q' - z' = q - z.  Whether an operand flips is read from its signed_flag on the
// device (asymmetric: always; symmetric: iff the byte is 0) into a mask register that every loaded dword is XORed with on its
// way into LDS (0 leaves signed codes as they are): no template parameter, one kernel.
//   The K tail.  mm_load_chunk zero-extends, and a flipped zero is -128.  The kernel flips EVERYTHING, padding included, and
// takes the padding out analytically: the pad count per row, npad = 128 nsteps - K, is the launch's, every pad byte of a
// flipping operand is p = -128 and of another 0, so the pads add px pw npad to S' and p npad to the operand's row sums.
// Flipping only the valid bytes would need a byte mask per chunk inside the step loop (the tail is any byte count); this way
// the loop has no tail case at all and the epilogue subtracts three launch-uniform products.
//
// Zero points without a second pass.  With S' = sum q'x q'w, R'x[m] = sum_k q'x, R'w[n] = sum_k q'w:
//   T = S' - z'w[n] R'x[m] - z'x[m] R'w[n] + K z'x[m] z'w[n]
// The row sums are accumulated inside the step loop from the fragments the lane holds anyway, by v_dot4 against 0x01010101:
// 8 per fragment, 64 per wave and step beside the 32 matrix instructions; no pre-pass, no workspace, no second read.  After the
// loop a lane has the sum of its row over its K group l / 16; two cross-lane additions (xor 16, xor 32) complete it in every
// lane.  R'x[m] is then in the lane that stores row m; the R'w[n + r] of register r is in the lanes l % 16 == 4 (l / 16) + r
// and comes by one shuffle each (16 per lane, epilogue only, before any lane is masked).
//   |S'| <= 2^14 * 2^15 = 2^29 (padded K <= 32768), row sums <= 2^22 and every term of the correction <= 2^29 in magnitude, but
// partial sums of the four can pass 2^31.  The correction is done in wrapping uint32: T itself satisfies |T| <= 255^2 K < 2^31
// for K <= 32768, so the low 32 bits read as int32 are T exactly.  When neither operand flips (signed symmetric x signed
// symmetric) every z' is 0 and there are no pads: the whole correction is skipped by a uniform branch.
//
// Epilogue.  scale = max(delta, eps) and zp = clamp(rint(zero_float), 0, 2^n - 1) (0 when symmetric) are the lane's own
// consts_of (fp8q_intq.h), read per row by the lanes that store it (index 0 when per tensor): 4 rows m and 16 rows n per
// lane.  y = float(T) * (sx * sw): the conversion rounds to nearest even, then two float32 multiplications; the unit is built
// with -ffp-contract=off and nothing here can fuse anyway.  A packed float32 multiplication rounds each half as the scalar
// form does, so the unit does not need the scalar-only flag the other products take.
//
// Rows past M / N are loaded as zeros, flipped or not, and never stored; their constants are never read.
#include "fp8q_intq.h"
#include "fp8q_mmq.h"

namespace {

using I8Panel = MmPanel<8>;
typedef int i4v __attribute__((ext_vector_type(4)));

constexpr int64_t kI8MaxK = 32768;      // 255^2 K < 2^31 up to here

struct I8Side {                 // one operand as fp8q_int_encode leaves it
    const uint8_t *codes;       // [rows, K]
    const float *delta;         // [1] or [rows]
    const float *zf;            // zero_float, as delta (asymmetric); unused when symmetric
    const unsigned char *sflag; // the device sign byte (symmetric); unused otherwise
    int64_t rows;
    int pc;                     // delta / zero_float have one entry per row
    int symmetric;
    float hi;                   // 2^n_bits - 1: where an asymmetric zero point clamps
    int w;                      // bytes per global load of the codes: 16, 8, 4 or 1
};

struct I8Args {
    I8Side x, w;                // the function's A (rows m) and B (rows n)
    void *y;
    int64_t K;
    int nsteps;                 // ceil(K / 128)
    int npad;                   // 128 nsteps - K: the zero bytes behind every row's last step
    float eps;
    int y_type;                 // FP8Q_DT_*
    int vec_store;              // N % 4 == 0 and y aligned to four of its elements
};

// what every dword of the operand's codes is XORed with: 0 for two's-complement codes, else the flip q -> q - 128
__device__ __forceinline__ uint32_t i8_flip(const I8Side &s) { return sign_byte(s.symmetric, s.sflag) ? 0u : 0x80808080u; }

template <class P>
__device__ __forceinline__ void i8_flip_panel(u4v (&g)[P::kPerLane], uint32_t mask)
{
#pragma unroll
    for (int j = 0; j < P::kPerLane; ++j) g[j] ^= mask;
}

// sum of the fragment's 32 signed bytes, added to r
__device__ __forceinline__ int i8_bytes_sum(const i8v f, int r)
{
#pragma unroll
    for (int d = 0; d < 8; ++d) r = __builtin_amdgcn_sdot4(f[d], 0x01010101, r, false);
    return r;
}

// scale and z' of row `row` (row < s.rows): the lane's consts_of, z' = zp - 128 under the flip
__device__ __forceinline__ void i8_row(const I8Side &s, int64_t row, bool flip, float eps, float &scale, uint32_t &z)
{
    const int64_t i = s.pc ? row : 0;
    const float4 k = consts_of(s.delta[i], s.symmetric ? 0.0f : s.zf[i], s.symmetric != 0, 0.0f, s.hi, eps);
    scale = k.x;
    z = (uint32_t)((int)k.z - (flip ? 128 : 0));
}

__global__ void __launch_bounds__(kMmBlock, 2)
k_i8mm(const I8Args a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_x[2][I8Panel::kBytes];
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][I8Panel::kBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;        // the wave's 64 x 64 quarter
    const int lr = lane & 15, lg = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.y * kMmTile, n0 = (int64_t)blockIdx.x * kMmTile;
    const uint32_t xflip = i8_flip(a.x), wflip = i8_flip(a.w);      // launch-uniform

    u4v gx[I8Panel::kPerLane], gw[I8Panel::kPerLane];
    i4v acc[4][4];      // [i: W's 16 rows][j: X's 16 rows]
    int rx[4], rw[4];   // the lane's share of the row sums of its X rows j and W rows i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rx[i] = rw[i] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = i4v{0, 0, 0, 0};
    }

    mm_load_panel<I8Panel, true>(gx, a.x.codes, a.K, a.x.rows, m0, 0, a.x.w, tid);
    mm_load_panel<I8Panel, true>(gw, a.w.codes, a.K, a.w.rows, n0, 0, a.w.w, tid);
    i8_flip_panel<I8Panel>(gx, xflip);
    i8_flip_panel<I8Panel>(gw, wflip);
    mm_store_panel<I8Panel>(s_x[0], gx, tid);
    mm_store_panel<I8Panel>(s_w[0], gw, tid);
    __syncthreads();

    for (int ks = 0; ks < a.nsteps; ++ks) {
        const int buf = ks & 1;
        const bool more = ks + 1 < a.nsteps;
        if (more) {         // the next step's loads fly over this step's instructions
            mm_load_panel<I8Panel, true>(gx, a.x.codes, a.K, a.x.rows, m0, ks + 1, a.x.w, tid);
            mm_load_panel<I8Panel, true>(gw, a.w.codes, a.K, a.w.rows, n0, ks + 1, a.w.w, tid);
        }
        i8v fw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fw[i] = mm_read_frag<I8Panel>(s_w[buf], wn * 64 + 16 * i + lr, lg);
            rw[i] = i8_bytes_sum(fw[i], rw[i]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i8v fx = mm_read_frag<I8Panel>(s_x[buf], wm * 64 + 16 * j + lr, lg);
            rx[j] = i8_bytes_sum(fx, rx[j]);
            const i4v xlo = {fx[0], fx[1], fx[2], fx[3]}, xhi = {fx[4], fx[5], fx[6], fx[7]};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const i4v wlo = {fw[i][0], fw[i][1], fw[i][2], fw[i][3]}, whi = {fw[i][4], fw[i][5], fw[i][6], fw[i][7]};
                acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wlo, xlo, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(whi, xhi, acc[i][j], 0, 0, 0);
            }
        }
        if (more) {
            // the other buffer: every wave left it at the barrier that ended the step before
            i8_flip_panel<I8Panel>(gx, xflip);
            i8_flip_panel<I8Panel>(gw, wflip);
            mm_store_panel<I8Panel>(s_x[buf ^ 1], gx, tid);
            mm_store_panel<I8Panel>(s_w[buf ^ 1], gw, tid);
        }
        __syncthreads();
    }

    // ---- epilogue: T from S' and the row sums, then the two scales ----
    const bool corr = (xflip | wflip) != 0u;        // else every z' is 0 and nothing was padded with -128
    const uint32_t px = xflip ? (uint32_t)-128 : 0u, pw = wflip ? (uint32_t)-128 : 0u, npad = (uint32_t)a.npad;
    uint32_t rwn[4][4];     // R'w of the row n of register r of acc[i][.], pads taken out
    if (corr) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            rx[t] += __shfl_xor(rx[t], 16);
            rx[t] += __shfl_xor(rx[t], 32);
            rw[t] += __shfl_xor(rw[t], 16);
            rw[t] += __shfl_xor(rw[t], 32);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) rwn[i][r] = (uint32_t)__shfl(rw[i], 4 * lg + r) - pw * npad;
    }
    const int64_t M = a.x.rows, N = a.w.rows;
    const int64_t n = n0 + wn * 64 + 4 * lg;
    float sw[4][4];
    uint32_t zw[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sw[i][r] = 0.0f, zw[i][r] = 0u;
            if (n + 16 * i + r < N) i8_row(a.w, n + 16 * i + r, wflip != 0u, a.eps, sw[i][r], zw[i][r]);
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t m = m0 + wm * 64 + 16 * j + lr;
        if (m >= M) continue;
        float sx;
        uint32_t zx;
        i8_row(a.x, m, xflip != 0u, a.eps, sx, zx);
        const uint32_t rxm = (uint32_t)rx[j] - px * npad;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t ni = n + 16 * i;
            if (ni >= N) continue;
            f4v v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                uint32_t t = (uint32_t)acc[i][j][r];
                if (corr)   // wrapping uint32: the low 32 bits of the four terms' sum are T, |T| < 2^31
                    t = t - px * pw * npad - zw[i][r] * rxm - zx * rwn[i][r] + (uint32_t)a.K * zx * zw[i][r];
                v[r] = (float)(int)t * (sx * sw[i][r]);
            }
            const int64_t left = N - ni;
            mm_store4(a.y, a.y_type, m * N + ni, v, left < 4 ? (int)left : 4, a.vec_store != 0);
        }
    }
}

// ---- host side ----
int i8_side(I8Side &s, const uint8_t *codes, const float *delta, const float *zf, const unsigned char *sflag, int64_t n_delta,
            int n_bits, int symmetric, int64_t rows, int64_t K)
{
    if (!codes || !delta || (symmetric ? !sflag : !zf) || (n_delta != 1 && n_delta != rows)) return FP8Q_EINVAL;
    if ((uintptr_t)delta % 4 || (!symmetric && (uintptr_t)zf % 4)) return FP8Q_EINVAL;
    s.codes = codes, s.delta = delta, s.zf = zf, s.sflag = sflag;
    s.rows = rows;
    s.pc = n_delta != 1;
    s.symmetric = symmetric != 0;
    s.hi = ldexpf(1.0f, n_bits) - 1.0f;
    s.w = mm_load_width(codes, K);
    return FP8Q_OK;
}

}  // namespace

extern "C" {

int fp8q_i8mm_nt(const uint8_t *a_codes, const float *a_delta, const float *a_zero_float, const unsigned char *a_signed_flag,
                 int64_t a_n_delta, int a_n_bits, int a_symmetric, const uint8_t *b_codes, const float *b_delta,
                 const float *b_zero_float, const unsigned char *b_signed_flag, int64_t b_n_delta, int b_n_bits, int b_symmetric,
                 void *y, int64_t M, int64_t N, int64_t K, float eps, int y_type, fp8q_stream_t stream)
{
    if (a_n_bits < 2 || a_n_bits > 8 || b_n_bits < 2 || b_n_bits > 8) return FP8Q_EUNSUPPORTED;
    if (K <= 0 || M < 0 || N < 0) return FP8Q_EINVAL;
    if (K > kI8MaxK) return FP8Q_EUNSUPPORTED;
    const int ybytes = mm_y_bytes(y_type);
    if (!ybytes) return FP8Q_EINVAL;
    if (M == 0 || N == 0) return FP8Q_OK;
    I8Args a;
    if (int rc = i8_side(a.x, a_codes, a_delta, a_zero_float, a_signed_flag, a_n_delta, a_n_bits, a_symmetric, M, K)) return rc;
    if (int rc = i8_side(a.w, b_codes, b_delta, b_zero_float, b_signed_flag, b_n_delta, b_n_bits, b_symmetric, N, K)) return rc;
    if (!y || (uintptr_t)y % (uintptr_t)ybytes) return FP8Q_EINVAL;
    int64_t gm, gn;
    if (!mm_tile_grid(M, N, gm, gn)) return FP8Q_EINVAL;
    a.y = y;
    a.K = K;
    a.nsteps = (int)cdiv(K, kMmTile);
    a.npad = (int)(a.nsteps * (int64_t)kMmTile - K);
    a.eps = eps;
    a.y_type = y_type;
    a.vec_store = mm_vec_store(N, y, ybytes);
    hipLaunchKernelGGL(k_i8mm, dim3((unsigned)gn, (unsigned)gm), dim3(kMmBlock), 0, (hipStream_t)stream, a);
    return launch_rc();
}

}  // extern "C"
