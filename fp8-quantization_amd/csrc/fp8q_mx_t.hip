// fp8q_mx_t.hip -- the microscaling (MX) lane with the blocks along dim 0 (gfx950 only): the operands of x^T made from x as it
// lies.  x is [R, K], K contiguous; column c is cut into the blocks of rows [32j, min(32j + 32, R)), one E8M0 byte each, and the
// results are, byte for byte, what fp8q_mx.hip gives for the contiguous [K, R] tensor x^T (include/fp8q.h defines them so, and
// fp8q_mx.hip's header states the arithmetic; every device function of it comes from fp8q_mxq.h, one copy for both files):
//   encode_t    codes_t [K, R] (FP8) / [K, R / 2] (E2M1) / [K, 3R / 4] (FP6) and scales_t [K, ceil(R / 32)]
//   encode_both the row-wise operands of fp8q_mx_encode_* and the transposed ones, from one read of x
//   quantize_t  y[r][c] = decode of the transposed operands at [c][r], in x's own layout
// Only what packs codes along R needs a divisible R (E2M1: even, FP6: a multiple of 4; encode_both the same of K for its
// row-wise half).  quantize_t packs nothing and takes every R and K.
//
// k_mxt<OP, F, IN, OUT, NT>, the tile route: rows readable with 16-byte loads (K % 4 == 0 for fp32, K % 8 == 0 for half) and
// every pointer 16-byte aligned.  A workgroup of 256 lanes takes a tile of 128 rows x 64 columns.
//   lane <-> (rr = tid / 16, cg = tid % 16): the 8 consecutive rows 8 rr .. 8 rr + 7 of the 4 columns 4 cg .. 4 cg + 3, its
//           eight loads (16 bytes of fp32, 8 of half) issued before any arithmetic; rows past R and columns past K are zeros
//           in registers, never read
//   column maxima: in the lane over its 8 rows, then over the 4 lanes of a 32-row block -- rr = 4j .. 4j + 3 are the lanes l,
//           l + 16, l + 32, l + 48 of wave j, so two cross-lane steps on integers and no barrier: wave j owns block j of the tile
//   row-wise half of encode_both: a row's block of 32 columns is 8 neighbouring lanes, k_mx's three-step DPP fold; the lane
//           stores the codes of its 4 columns itself (a wave writes 4 rows x 64 bytes of FP8 with one instruction)
//   transposed codes: a lane converts its elements under its columns' scales and packs the 8 rows of a column in registers
//           (8 bytes of FP8, 6 of FP6, 4 of FP4: E2M1 and FP6 pack neighbouring ROWS, which the lane holds).  Those chunks --
//           codes, not values -- go through LDS as [column][run of the tile's 128 rows] and leave as 16-byte words along R:
//           consecutive lanes write one column's 128 (96, 64) contiguous bytes.  16-byte words need a codes_t row of a
//           multiple of 16 bytes; a multiple of 4 is stored dword by dword, anything else byte by byte (fp8q_mxt_route
//           reports which), as is the short last word of a short last tile
//   scale bytes: the tile's 4 blocks of a column are gathered in LDS and leave as one dword per column (byte by byte where
//           ceil(R / 32) is no multiple of 4 or the tile is the short last one)
//   quantize_t needs no LDS: the values leave at the addresses the elements came from
// LDS layout and its bank conflicts by the rule bank = (byte address / 4) mod 32 per 32-lane half (every ds_write, ds_read_b32):
// a column's run starts every kPitch = run + 4 bytes (132 / 100 / 68: 33 / 25 / 17 dwords, odd), the chunk of lane rr at byte
// rr * chunk.  Writes, dword (FP8, FP4) or 16-bit (FP6) stores: the 16 lanes cg of a half-wave step 4 columns = 4 dwords mod 32
// apart, so cg and cg + 8 meet on a bank and nothing else does -- 2-way, which a ds_write's own issue time covers.  Reads, four
// dword loads per 16-byte word: a half-wave reads 4 (FP8) / 8 (FP4) columns x all their words at dwords column + 4 part + i mod
// 32 -- FP8 conflict-free, FP4 2-way (column + 4 and part + 1 meet), FP6 (6 words a column, 5 columns and a third per half-wave)
// at most 2-way.  The LDS moves 1 byte per element here against 4 + 1 of HBM traffic; none of this is near a limit.
// Every element of x is read from HBM exactly once.  NT: nontemporal loads and stores from 64 MiB (kNtBytes), the lane's rule.
// k_mxt_plain<OP, F, IN, OUT>, the general route (ragged or odd K, misaligned views): one lane per block, its elements K apart
// (consecutive lanes take consecutive columns), four at a time; encode_both gives the row-wise blocks lanes of their own, so
// that route reads x twice.  The twin of k_mx_plain: a correctness path, no rate is claimed for it.
// One launch per call, nothing read back, no allocation, no workspace.  gfx950's scaled conversions are not used, for the
// reason fp8q_mx.hip gives.
#include "fp8q_common.h"
#include "fp8q_io.h"
#include "fp8q_mxq.h"

namespace {

enum { kOpT, kOpBoth, kOpQuantT };     // encode_t, encode_both, quantize_t

constexpr int kTileRows = 128;         // 4 waves x one block of 32 rows
constexpr int kTileCols = 64;          // 16 lanes x 4 columns
constexpr int kLaneRows = 8;

// bits of a code, bytes of a lane's 8 rows of one column, of a tile's 128 rows, and from one column's run to the next in LDS
template <int F>
constexpr int kBits = F == FP8Q_MX_E2M1 ? 4 : (kFp6<F> ? 6 : 8);
template <int F>
constexpr int kChunk = kLaneRows * kBits<F> / 8;
template <int F>
constexpr int kRun = kTileRows * kBits<F> / 8;
template <int F>
constexpr int kPitch = kRun<F> + 4;

struct MxtArgs {
    uint8_t *codes, *scales;          // the row-wise operands (encode_both)
    uint8_t *codes_t, *scales_t;      // the transposed ones
    int64_t R, K;
    int64_t nbR, nbK;                 // blocks per column, per row
    int64_t pitch_t;                  // bytes of a row of codes_t
    int64_t tilesC;                   // tiles per 128 rows
    int ceil_rule;
    int gran;                         // bytes per store of transposed codes: 16, 4 or 1
    MxSr sr;                          // the SR kernels' seed and offset
};

// one tile's transposed codes from LDS (s) to codes_t (dst: the tile's first byte), G bytes per store; run: the bytes of a
// column that are rows of the tensor, ncols: the columns that are
template <int F, int G, bool NT>
__device__ __forceinline__ void store_runs(const uint8_t *s, uint8_t *dst, int64_t pitch, int run, int ncols, int tid)
{
    constexpr int UPC = kRun<F> / G;            // stores per column of a full tile
    for (int u = tid; u < kTileCols * UPC; u += kBlock) {
        const int col = u / UPC, off = (u - col * UPC) * G;
        if (col >= ncols || off >= run) continue;
        const uint8_t *src = s + col * kPitch<F> + off;
        uint8_t *d = dst + col * pitch + off;
        if (off + G <= run) {
            if constexpr (G == 16) {
                const uint32_t *w = reinterpret_cast<const uint32_t *>(src);
                stv<NT>(reinterpret_cast<u4v *>(d), u4v{w[0], w[1], w[2], w[3]});
            } else if constexpr (G == 4) {
                stv<NT>(reinterpret_cast<uint32_t *>(d), *reinterpret_cast<const uint32_t *>(src));
            } else {
                *d = *src;
            }
        } else {
            for (int i = 0; off + i < run; ++i) d[i] = src[i];      // the short last word of a short last tile
        }
    }
}

// ---- the tile route ----
// SR: elem = RNE(SR(q, r)), the draws by the element's flat index in x as it lies (fp8q_mxq.h): the 4 columns of a lane's row
// are an aligned group of four (K % 4 == 0, the offset a multiple of 8), half a Philox call, made once and used by the
// transposed codes and by encode_both's row-wise ones alike
template <int OP, int F, class IN, class OUT, bool NT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_mxt(const void *__restrict__ in, void *__restrict__ out, MxtArgs a)
{
    typedef typename IN::elem in_t;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[OP == kOpQuantT ? 16 : kTileCols * kPitch<F>];
    __shared__ uint32_t s_scales[kTileCols];
    const int tid = threadIdx.x, cg = tid & 15, rr = tid >> 4;
    const int64_t tr = (int64_t)blockIdx.x / a.tilesC, tc = (int64_t)blockIdx.x - tr * a.tilesC;
    const int64_t r0 = tr * kTileRows, c0 = tc * kTileCols;
    const int64_t c = c0 + 4 * cg, row0 = r0 + kLaneRows * rr;
    const bool col_live = c < a.K;             // K % 4 == 0: the lane's 4 columns exist together
    const in_t *x = static_cast<const in_t *>(in);
    float v[kLaneRows][4];
#pragma unroll
    for (int p = 0; p < kLaneRows; ++p) {
        v[p][0] = v[p][1] = v[p][2] = v[p][3] = 0.0f;
        if (col_live && row0 + p < a.R) IN::template load4<NT>(x + (row0 + p) * a.K + c, v[p]);
    }
    // the scale byte of each of the lane's columns: every lane of the wave runs the two cross-lane steps
    uint32_t sct[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t m = 0u;
#pragma unroll
        for (int p = 0; p < kLaneRows; ++p) {
            const uint32_t t = abs_bits(v[p][k]);
            m = t > m ? t : m;
        }
        uint32_t o = (uint32_t)__shfl_xor((int)m, 16);
        m = o > m ? o : m;
        o = (uint32_t)__shfl_xor((int)m, 32);
        m = o > m ? o : m;
        sct[k] = scale_code<F>(m, a.ceil_rule);
    }
    // the two draw words of each of the lane's rows: columns 0, 1 in the first, 2, 3 in the second
    uint32_t dr[SR ? kLaneRows : 1][2];
    if constexpr (SR) {
#pragma unroll
        for (int p = 0; p < kLaneRows; ++p)
            mx_draw4(a.sr, a.sr.offset + (uint64_t)(row0 + p) * (uint64_t)a.K + (uint64_t)c, dr[p]);
    }
    // the codes of the lane's rows 4h .. 4h + 3 of column k
    uint32_t wt[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float t[4] = {v[4 * h][k], v[4 * h + 1][k], v[4 * h + 2][k], v[4 * h + 3][k]};
            if constexpr (SR) {
                uint32_t r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = (dr[4 * h + i][k >> 1] >> (16 * (k & 1))) & 0xffffu;
                wt[k][h] = mx_code4_sr<F>(t, sct[k], r);
            } else {
                wt[k][h] = mx_code4<F>(t, sct[k]);
            }
        }
    }
    if constexpr (OP == kOpQuantT) {
        typedef typename OUT::elem out_t;
        out_t *y = static_cast<out_t *>(out);
        float r[kLaneRows][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float t[4];
                mx_value4<F>(wt[k][h], sct[k], t);
#pragma unroll
                for (int i = 0; i < 4; ++i) r[4 * h + i][k] = t[i];
            }
        }
#pragma unroll
        for (int p = 0; p < kLaneRows; ++p)
            if (col_live && row0 + p < a.R) OUT::template store4<NT>(y + (row0 + p) * a.K + c, r[p]);
    } else {
        // the chunks of the lane's 4 columns into LDS (zeros where the tensor ends: they are not stored from there)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint8_t *s = s_codes + (4 * cg + k) * kPitch<F> + rr * kChunk<F>;
            if constexpr (F == FP8Q_MX_E2M1) {
                *reinterpret_cast<uint32_t *>(s) = wt[k][0] | (wt[k][1] << 16);
            } else if constexpr (kFp6<F>) {
                uint16_t *s2 = reinterpret_cast<uint16_t *>(s);
                s2[0] = (uint16_t)wt[k][0];
                s2[1] = (uint16_t)((wt[k][0] >> 16) | (wt[k][1] << 8));
                s2[2] = (uint16_t)(wt[k][1] >> 8);
            } else {
                uint32_t *s4 = reinterpret_cast<uint32_t *>(s);
                s4[0] = wt[k][0];
                s4[1] = wt[k][1];
            }
            if (!(rr & 3)) reinterpret_cast<uint8_t *>(s_scales)[4 * (4 * cg + k) + (rr >> 2)] = (uint8_t)sct[k];
        }
        if constexpr (OP == kOpBoth) {
            // the row-wise operands: the lanes 8i .. 8i + 7 hold 32 columns of a row; every lane runs the folds
#pragma unroll
            for (int p = 0; p < kLaneRows; ++p) {
                uint32_t m = umax4(v[p]);
                m = umax_xor<1>(m);
                m = umax_xor<2>(m);
                m = umax_xor<4>(m);
                const uint32_t sc = scale_code<F>(m, a.ceil_rule);
                uint32_t w;
                if constexpr (SR) {
                    uint32_t r[4];
                    mx_split4(dr[p], r);
                    w = mx_code4_sr<F>(v[p], sc, r);
                } else {
                    w = mx_code4<F>(v[p], sc);
                }
                const int64_t row = row0 + p;
                if (col_live && row < a.R) {
                    const int64_t e = row * a.K + c;
                    if constexpr (F == FP8Q_MX_E2M1) {
                        stv<NT>(reinterpret_cast<uint16_t *>(a.codes + (e >> 1)), (uint16_t)w);
                    } else if constexpr (kFp6<F>) {
                        uint8_t *d = a.codes + 3 * (e >> 2);
                        d[0] = (uint8_t)w;
                        d[1] = (uint8_t)(w >> 8);
                        d[2] = (uint8_t)(w >> 16);
                    } else {
                        stv<NT>(reinterpret_cast<uint32_t *>(a.codes + e), w);
                    }
                    if (!(cg & 7)) a.scales[row * a.nbK + (c >> 5)] = (uint8_t)sc;
                }
            }
        }
        __syncthreads();
        const int rows = (int)(a.R - r0 < kTileRows ? a.R - r0 : kTileRows);
        const int ncols = (int)(a.K - c0 < kTileCols ? a.K - c0 : kTileCols);
        const int run = rows * kBits<F> / 8;       // whole bytes: E2M1 has an even R, FP6 a multiple of 4
        uint8_t *dst = a.codes_t + c0 * a.pitch_t + r0 * kBits<F> / 8;
        if (a.gran == 16) store_runs<F, 16, NT>(s_codes, dst, a.pitch_t, run, ncols, tid);
        else if (a.gran == 4) store_runs<F, 4, NT>(s_codes, dst, a.pitch_t, run, ncols, tid);
        else store_runs<F, 1, NT>(s_codes, dst, a.pitch_t, run, ncols, tid);
        if (tid < ncols) {
            const int64_t left = a.nbR - 4 * tr;
            uint8_t *d = a.scales_t + (c0 + tid) * a.nbR + 4 * tr;
            if (left >= 4 && !(a.nbR & 3)) {
                stv<NT>(reinterpret_cast<uint32_t *>(d), s_scales[tid]);
            } else {
                const uint32_t w = s_scales[tid];
                for (int i = 0; i < 4 && i < left; ++i) d[i] = (uint8_t)(w >> (8 * i));
            }
        }
    }
}

// ---- the general route: one lane per block ----
// the block of `len` elements `stride` apart from x[base]: its scale byte to *scale_at and its codes from codes_at on (encode),
// or its values to y at the elements' own places (quantize); four elements at a time, the last group may be short
template <bool QUANT, int F, class IN, class OUT, bool SR>
__device__ __forceinline__ void plain_block(const typename IN::elem *x, typename OUT::elem *y, int64_t base, int64_t stride,
                                            int len, int ceil_rule, uint8_t *codes_at, uint8_t *scale_at, const MxSr &sr)
{
    uint32_t m = 0u;
    for (int i = 0; i < len; ++i) {
        const uint32_t t = abs_bits(IN::load1(x + base + i * stride));
        m = t > m ? t : m;
    }
    const uint32_t sc = scale_code<F>(m, ceil_rule);
    if constexpr (!QUANT) *scale_at = (uint8_t)sc;
    for (int i = 0; i < len; i += 4) {
        const int nv = len - i < 4 ? len - i : 4;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nv) v[k] = IN::load1(x + base + (i + k) * stride);
        uint32_t w;
        if constexpr (SR) {
            uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) r[k] = mx_draw1(sr, sr.offset + (uint64_t)(base + (i + k) * stride));
            w = mx_code4_sr<F>(v, sc, r);
        } else {
            w = mx_code4<F>(v, sc);
        }
        if constexpr (QUANT) {
            float r[4];
            mx_value4<F>(w, sc, r);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) OUT::store1(y + base + (i + k) * stride, r[k]);
        } else {
            // whole bytes: an E2M1 block has an even length, an FP6 block a multiple of 4 (the launcher has checked)
            const int nbytes = nv * kBits<F> / 8;
            uint8_t *cb = codes_at + i * kBits<F> / 8;
            for (int k = 0; k < nbytes; ++k) cb[k] = (uint8_t)(w >> (8 * k));
        }
    }
}

template <int OP, int F, class IN, class OUT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_mxt_plain(const void *__restrict__ in, void *__restrict__ out, MxtArgs a)
{
    typedef typename IN::elem in_t;
    const in_t *x = static_cast<const in_t *>(in);
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t tblocks = a.K * a.nbR;
    if (b < tblocks) {
        const int64_t j = b / a.K, c = b - j * a.K;        // consecutive lanes: consecutive columns
        const int len = (int)(a.R - kMxBlock * j < kMxBlock ? a.R - kMxBlock * j : kMxBlock);
        if constexpr (OP == kOpQuantT) {
            plain_block<true, F, IN, OUT, SR>(x, static_cast<typename OUT::elem *>(out), kMxBlock * j * a.K + c, a.K, len,
                                              a.ceil_rule, nullptr, nullptr, a.sr);
        } else {
            plain_block<false, F, IN, IoF32, SR>(x, nullptr, kMxBlock * j * a.K + c, a.K, len, a.ceil_rule,
                                                 a.codes_t + c * a.pitch_t + kMxBlock * j * kBits<F> / 8,
                                                 a.scales_t + c * a.nbR + j, a.sr);
        }
    } else if constexpr (OP == kOpBoth) {
        const int64_t b2 = b - tblocks;
        if (b2 >= a.R * a.nbK) return;
        const int64_t row = b2 / a.nbK, j = b2 - row * a.nbK;
        const int len = (int)(a.K - kMxBlock * j < kMxBlock ? a.K - kMxBlock * j : kMxBlock);
        plain_block<false, F, IN, IoF32, SR>(x, nullptr, row * a.K + kMxBlock * j, 1, len, a.ceil_rule,
                                             a.codes + (row * a.K + kMxBlock * j) * kBits<F> / 8, a.scales + b2, a.sr);
    }
}

inline bool fmt_known(int fmt)
{
    return fmt == FP8Q_MX_E4M3FN || fmt == FP8Q_MX_E5M2 || fmt == FP8Q_MX_E2M1 || fmt == FP8Q_MX_E2M3 || fmt == FP8Q_MX_E3M2;
}

inline int fmt_bits(int fmt) { return fmt == FP8Q_MX_E2M1 ? 4 : ((fmt == FP8Q_MX_E2M3 || fmt == FP8Q_MX_E3M2) ? 6 : 8); }

// THE launch rule of the three entries: which kernel, with which hints and which store width.  Arguments are the caller's
// business except where a wrong one would make the arithmetic below meaningless.
int mxt_route(int64_t R, int64_t K, int fmt, int x_type, int aligned16, fp8q_mxt_route_info *info)
{
    if (!info || R <= 0 || K <= 0) return FP8Q_EINVAL;
    if (!fmt_known(fmt)) return FP8Q_EUNSUPPORTED;
    if (x_type != FP8Q_DT_F32 && !half_type(x_type)) return FP8Q_EINVAL;
    if (R > INT64_MAX / K) return FP8Q_EINVAL;
    const int per16 = x_type == FP8Q_DT_F32 ? 4 : 8;       // elements of a 16-byte load
    const bool tile = aligned16 && K % per16 == 0;
    const int64_t bits = fmt_bits(fmt);
    const int64_t pitch = R * bits / 8;                     // (meaningful where R packs into whole bytes: the encoders)
    fp8q_mxt_route_info r = {};
    r.kernel = tile ? FP8Q_MXT_TILE : FP8Q_MXT_GENERAL;
    r.tile_rows = kTileRows;
    r.tile_cols = kTileCols;
    r.nontemporal = tile && R * K >= kNtBytes / 4;
    r.code_store_bytes = !tile ? 1 : (pitch % 16 == 0 ? 16 : (pitch % 4 == 0 ? 4 : 1));
    *info = r;
    return FP8Q_OK;
}

// Argument checks (everything is reported before the launch, in mx_launch's order and with its codes) and the one launch.
// x_type / y_type: FP8Q_DT_*; y and y_type are quantize_t's, the four operand pointers the encoders'.  sr: the seed and offset
// of a stochastic-rounding entry, null for round to nearest even.
template <int OP>
int mxt_launch(const void *x, void *y, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int x_type,
               int y_type, int64_t R, int64_t K, int fmt, int rounding, hipStream_t st, const MxSr *sr = nullptr)
{
    constexpr bool enc = OP != kOpQuantT;
    if (!x || (enc && (!codes_t || !scales_t)) || (OP == kOpBoth && (!codes || !scales)) || (!enc && !y) || R <= 0 || K <= 0)
        return FP8Q_EINVAL;
    if (!fmt_known(fmt)) return FP8Q_EUNSUPPORTED;
    if (rounding != FP8Q_MX_FLOOR && rounding != FP8Q_MX_CEIL) return FP8Q_EINVAL;
    if (sr && (sr->offset & 7u)) return FP8Q_EINVAL;
    const int bits = fmt_bits(fmt);
    const int64_t mult = bits == 4 ? 2 : (bits == 6 ? 4 : 1);         // elements that share whole bytes
    if (enc && R % mult) return FP8Q_EINVAL;
    if (OP == kOpBoth && K % mult) return FP8Q_EINVAL;
    if (value_side_misaligned(x, x_type) || (!enc && value_side_misaligned(y, y_type))) return FP8Q_EINVAL;
    const int64_t nbR = cdiv(R, kMxBlock), nbK = cdiv(K, kMxBlock);
    if (R > INT64_MAX / K || K > INT64_MAX / nbR / 2 || R > INT64_MAX / nbK / 2) return FP8Q_EINVAL;
    const uintptr_t ptrs = (uintptr_t)x | (uintptr_t)y | (uintptr_t)codes | (uintptr_t)scales | (uintptr_t)codes_t |
                           (uintptr_t)scales_t;                       // (the entries pass null for what they do not take)
    fp8q_mxt_route_info route;
    if (int rc = mxt_route(R, K, fmt, x_type, (ptrs & 15) == 0, &route)) return rc;
    const bool tile = route.kernel == FP8Q_MXT_TILE;
    const int64_t tilesR = cdiv(R, kTileRows), tilesC = cdiv(K, kTileCols);
    const int64_t lanes = K * nbR + (OP == kOpBoth ? R * nbK : 0);
    const int64_t grid = tile ? (tilesR > (int64_t)INT32_MAX / tilesC ? (int64_t)INT32_MAX + 1 : tilesR * tilesC)
                              : cdiv(lanes, kBlock);
    if (grid > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    MxtArgs a = {};
    a.codes = codes;
    a.scales = scales;
    a.codes_t = codes_t;
    a.scales_t = scales_t;
    a.R = R;
    a.K = K;
    a.nbR = nbR;
    a.nbK = nbK;
    a.pitch_t = R * bits / 8;
    a.tilesC = tilesC;
    a.ceil_rule = rounding == FP8Q_MX_CEIL;
    a.gran = route.code_store_bytes;
    if (sr) a.sr = *sr;
    const dim3 g((unsigned)grid), b(kBlock);
    auto run = [&](auto fc, auto in, auto outp, auto sr_on) {
        constexpr int F = decltype(fc)::value;
        constexpr bool SR = decltype(sr_on)::value;
        typedef decltype(in) IN;
        typedef decltype(outp) OUT;
        if (!tile) hipLaunchKernelGGL((k_mxt_plain<OP, F, IN, OUT, SR>), g, b, 0, st, x, y, a);
        else if (route.nontemporal) hipLaunchKernelGGL((k_mxt<OP, F, IN, OUT, true, SR>), g, b, 0, st, x, y, a);
        else hipLaunchKernelGGL((k_mxt<OP, F, IN, OUT, false, SR>), g, b, 0, st, x, y, a);
    };
    auto go = [&](auto fc, auto in, auto outp) {
        if (sr) run(fc, in, outp, std::true_type{});
        else run(fc, in, outp, std::false_type{});
    };
    dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M3, FP8Q_MX_E3M2, FP8Q_MX_E2M1>(fmt, [&](auto fc) {
        value_io(x_type, [&](auto in) {
            if constexpr (enc) {
                go(fc, in, IoCodes{});
            } else {
                if (y_type == FP8Q_DT_F32) go(fc, in, IoF32{});
                else go(fc, in, in);
            }
        });
    });
    return launch_rc();
}

}  // namespace

extern "C" {

int fp8q_mxt_route(int64_t R, int64_t K, int fmt, int x_type, int aligned16, fp8q_mxt_route_info *info)
{
    return mxt_route(R, K, fmt, x_type, aligned16, info);
}

int fp8q_mxt_encode_f32(const float *x, uint8_t *codes_t, uint8_t *scales_t, int64_t R, int64_t K, int fmt, int rounding,
                        fp8q_stream_t stream)
{
    return mxt_launch<kOpT>(x, nullptr, nullptr, nullptr, codes_t, scales_t, FP8Q_DT_F32, -1, R, K, fmt, rounding,
                            (hipStream_t)stream);
}

int fp8q_mxt_encode_h16(const void *x, uint8_t *codes_t, uint8_t *scales_t, int x_type, int64_t R, int64_t K, int fmt,
                        int rounding, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    return mxt_launch<kOpT>(x, nullptr, nullptr, nullptr, codes_t, scales_t, x_type, -1, R, K, fmt, rounding,
                            (hipStream_t)stream);
}

int fp8q_mxt_encode_both_f32(const float *x, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int64_t R,
                             int64_t K, int fmt, int rounding, fp8q_stream_t stream)
{
    return mxt_launch<kOpBoth>(x, nullptr, codes, scales, codes_t, scales_t, FP8Q_DT_F32, -1, R, K, fmt, rounding,
                               (hipStream_t)stream);
}

int fp8q_mxt_encode_both_h16(const void *x, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int x_type,
                             int64_t R, int64_t K, int fmt, int rounding, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    return mxt_launch<kOpBoth>(x, nullptr, codes, scales, codes_t, scales_t, x_type, -1, R, K, fmt, rounding,
                               (hipStream_t)stream);
}

int fp8q_mxt_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, fp8q_stream_t stream)
{
    return mxt_launch<kOpQuantT>(x, y, nullptr, nullptr, nullptr, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, fmt, rounding,
                                 (hipStream_t)stream);
}

int fp8q_mxt_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                          fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    return mxt_launch<kOpQuantT>(x, y, nullptr, nullptr, nullptr, nullptr, x_type, y_type, R, K, fmt, rounding,
                                 (hipStream_t)stream);
}

// ---- stochastic rounding of the elements: the twins of the six launching entries above ----
int fp8q_mxsr_encode_t_f32(const float *x, uint8_t *codes_t, uint8_t *scales_t, int64_t R, int64_t K, int fmt, int rounding,
                           uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return mxt_launch<kOpT>(x, nullptr, nullptr, nullptr, codes_t, scales_t, FP8Q_DT_F32, -1, R, K, fmt, rounding,
                            (hipStream_t)stream, &sr);
}

int fp8q_mxsr_encode_t_h16(const void *x, uint8_t *codes_t, uint8_t *scales_t, int x_type, int64_t R, int64_t K, int fmt,
                           int rounding, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    const MxSr sr = mx_sr_args(seed, offset);
    return mxt_launch<kOpT>(x, nullptr, nullptr, nullptr, codes_t, scales_t, x_type, -1, R, K, fmt, rounding,
                            (hipStream_t)stream, &sr);
}

int fp8q_mxsr_encode_both_f32(const float *x, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int64_t R,
                              int64_t K, int fmt, int rounding, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return mxt_launch<kOpBoth>(x, nullptr, codes, scales, codes_t, scales_t, FP8Q_DT_F32, -1, R, K, fmt, rounding,
                               (hipStream_t)stream, &sr);
}

int fp8q_mxsr_encode_both_h16(const void *x, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int x_type,
                              int64_t R, int64_t K, int fmt, int rounding, uint64_t seed, uint64_t offset,
                              fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    const MxSr sr = mx_sr_args(seed, offset);
    return mxt_launch<kOpBoth>(x, nullptr, codes, scales, codes_t, scales_t, x_type, -1, R, K, fmt, rounding,
                               (hipStream_t)stream, &sr);
}

int fp8q_mxsr_quantize_t_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, uint64_t seed,
                             uint64_t offset, fp8q_stream_t stream)
{
    const MxSr sr = mx_sr_args(seed, offset);
    return mxt_launch<kOpQuantT>(x, y, nullptr, nullptr, nullptr, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, fmt, rounding,
                                 (hipStream_t)stream, &sr);
}

int fp8q_mxsr_quantize_t_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                             uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    const MxSr sr = mx_sr_args(seed, offset);
    return mxt_launch<kOpQuantT>(x, y, nullptr, nullptr, nullptr, nullptr, x_type, y_type, R, K, fmt, rounding,
                                 (hipStream_t)stream, &sr);
}

}  // extern "C"
