// fp8q_mx_had_t.hip -- the MX lane with a block Hadamard rotation in front of the quantization, blocks along dim 0 (gfx950
// only).  x is [R, K], K contiguous, R % 32 == 0; the results are, byte for byte, what fp8q_mx_had.hip gives for the contiguous
// [K, R] tensor x^T (quantize_t: transposed back, so y lies as x does).  The rotation is fp8q_hadq.h's, everything after it
// fp8q_mxq.h's, and the tile, its LDS layout and the code stores are k_mxt's (fp8q_mxtq.h; fp8q_mx_t.hip's header explains them).
//
// k_mxth<QUANT, F, IN, OUT, NT, SR>, the tile route (fp8q_mxt_route's rule, unchanged): 256 lanes on 128 rows x 64 columns, a
// lane holding the 8 consecutive rows 8 rr .. 8 rr + 7 of 4 columns, its eight loads issued before any arithmetic.  A 32-row
// block of a column is the four lanes l, l + 16, l + 32, l + 48 of one wave, so for each of the lane's 4 columns:
//   signs: the 8 bits of the mask at 8 (rr & 3); stages 0 .. 2 in registers over the lane's 8 rows; stages 3 and 4 one exchange
//   each with the lanes 16 and 32 away (ds_bpermute, as the column maxima); the multiplication
// then the integer maxima, scale_code, mx_code4 / mx_code4_sr as k_mxt runs them, and
//   encode_t:   the codes of the lane's 8 rows of a column through LDS ([column][run of 128 rows], odd dword pitch) and out as
//               16 / 4 / 1-byte stores along R, the scale bytes of a tile's 4 blocks as one dword per column
//   quantize_t: the values, the inverse rotation the same way back, and the stores at the addresses the elements came from
// Rows past R are whole blocks (R % 32 == 0) and columns past K whole lanes: zeros in registers, never read, never stored.
// k_mxth_plain, the general route (odd K, misaligned views): one lane per block, its 32 values K apart in registers, all five
// stages in the lane; consecutive lanes take consecutive columns.  A correctness path, as k_mxt_plain is.
// The draws of stochastic rounding go by the element's flat index in x as it lies, which the rotation does not move.
#include "fp8q_common.h"
#include "fp8q_hadq.h"
#include "fp8q_io.h"
#include "fp8q_mxq.h"
#include "fp8q_mxtq.h"

namespace {

struct MxthArgs {
    MxtArgs t;
    uint32_t mask;
};

// the rotation of the lane's 8 rows x 4 columns: signs `pre` before, signs `post` after (the lane's 8 bits of the mask)
__device__ __forceinline__ void had_tile(float (*v)[4], uint32_t pre, uint32_t post, int rr)
{
    float *f = &v[0][0];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        had_signs<kLaneRows, 4>(f + k, pre);
        had_regs<kLaneRows, 4>(f + k);
    }
    had_cross<16, 4 * kLaneRows>(f, (uint32_t)(rr & 1) << 31);
    had_cross<32, 4 * kLaneRows>(f, (uint32_t)(rr & 2) << 30);
    had_norm<4 * kLaneRows>(f);
#pragma unroll
    for (int k = 0; k < 4; ++k) had_signs<kLaneRows, 4>(f + k, post);
}

template <bool QUANT, int F, class IN, class OUT, bool NT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_mxth(const void *__restrict__ in, void *__restrict__ out, MxthArgs ha)
{
    typedef typename IN::elem in_t;
    const MxtArgs &a = ha.t;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[QUANT ? 16 : kTileCols * kPitch<F>];
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
    const uint32_t sb = (ha.mask >> (kLaneRows * (rr & 3))) & 0xffu;
    had_tile(v, sb, 0u, rr);
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
    if constexpr (QUANT) {
        typedef typename OUT::elem out_t;
        out_t *y = static_cast<out_t *>(out);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float t[4];
                mx_value4<F>(wt[k][h], sct[k], t);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[4 * h + i][k] = t[i];
            }
        }
        had_tile(v, 0u, sb, rr);
#pragma unroll
        for (int p = 0; p < kLaneRows; ++p)
            if (col_live && row0 + p < a.R) OUT::template store4<NT>(y + (row0 + p) * a.K + c, v[p]);
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
        __syncthreads();
        const int rows = (int)(a.R - r0 < kTileRows ? a.R - r0 : kTileRows);
        const int ncols = (int)(a.K - c0 < kTileCols ? a.K - c0 : kTileCols);
        const int run = rows * kBits<F> / 8;
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

// ---- the general route: one lane per block, its 32 elements K apart ----
template <bool QUANT, int F, class IN, class OUT, bool SR>
__global__ void __launch_bounds__(kBlock)
k_mxth_plain(const void *__restrict__ in, void *__restrict__ out, MxthArgs ha)
{
    typedef typename IN::elem in_t;
    const MxtArgs &a = ha.t;
    const in_t *x = static_cast<const in_t *>(in);
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= a.K * a.nbR) return;
    const int64_t j = b / a.K, c = b - j * a.K;        // consecutive lanes: consecutive columns
    const int64_t base = kMxBlock * j * a.K + c;
    float v[kMxBlock];
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i) v[i] = IN::load1(x + base + i * a.K);
    had_block32(v, ha.mask, 0u);
    uint32_t m = 0u;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const uint32_t t = umax4(v + 4 * g);
        m = t > m ? t : m;
    }
    const uint32_t sc = scale_code<F>(m, a.ceil_rule);
    constexpr int kBytes = kBits<F> / 2;                    // code bytes of a group of 4
    if constexpr (!QUANT) a.scales_t[c * a.nbR + j] = (uint8_t)sc;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        uint32_t w;
        if constexpr (SR) {
            uint32_t r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = mx_draw1(a.sr, a.sr.offset + (uint64_t)(base + (4 * g + k) * a.K));
            w = mx_code4_sr<F>(v + 4 * g, sc, r);
        } else {
            w = mx_code4<F>(v + 4 * g, sc);
        }
        if constexpr (QUANT) {
            mx_value4<F>(w, sc, v + 4 * g);
        } else {
            uint8_t *cb = a.codes_t + c * a.pitch_t + (8 * j + g) * kBytes;
#pragma unroll
            for (int k = 0; k < kBytes; ++k) cb[k] = (uint8_t)(w >> (8 * k));
        }
    }
    if constexpr (QUANT) {
        typedef typename OUT::elem out_t;
        out_t *y = static_cast<out_t *>(out);
        had_block32(v, 0u, ha.mask);
#pragma unroll
        for (int i = 0; i < kMxBlock; ++i) OUT::store1(y + base + i * a.K, v[i]);
    }
}

// Argument checks (everything is reported before the launch, in mxt_launch's order and with its codes) and the one launch.
template <bool QUANT>
int mxth_launch(const void *x, void *y, uint8_t *codes_t, uint8_t *scales_t, int x_type, int y_type, int64_t R, int64_t K,
                int fmt, int rounding, uint32_t mask, hipStream_t st, const MxSr *sr)
{
    if (!x || (!QUANT && (!codes_t || !scales_t)) || (QUANT && !y) || R <= 0 || K <= 0) return FP8Q_EINVAL;
    const bool fp6 = fmt == FP8Q_MX_E2M3 || fmt == FP8Q_MX_E3M2;
    if (fmt != FP8Q_MX_E4M3FN && fmt != FP8Q_MX_E5M2 && fmt != FP8Q_MX_E2M1 && !fp6) return FP8Q_EUNSUPPORTED;
    if (rounding != FP8Q_MX_FLOOR && rounding != FP8Q_MX_CEIL) return FP8Q_EINVAL;
    if (sr && (sr->offset & 7u)) return FP8Q_EINVAL;
    if (R % kMxBlock) return FP8Q_EINVAL;                   // blocks are never short under a rotation
    if (value_side_misaligned(x, x_type) || (QUANT && value_side_misaligned(y, y_type))) return FP8Q_EINVAL;
    const int64_t nbR = R / kMxBlock;
    if (R > INT64_MAX / K || K > INT64_MAX / nbR / 2) return FP8Q_EINVAL;
    const uintptr_t ptrs = (uintptr_t)x | (uintptr_t)y | (uintptr_t)codes_t | (uintptr_t)scales_t;
    fp8q_mxt_route_info route;
    if (int rc = fp8q_mxt_route(R, K, fmt, x_type, (ptrs & 15) == 0, &route)) return rc;
    const bool tile = route.kernel == FP8Q_MXT_TILE;
    const int64_t tilesR = cdiv(R, kTileRows), tilesC = cdiv(K, kTileCols);
    const int64_t grid = tile ? (tilesR > (int64_t)INT32_MAX / tilesC ? (int64_t)INT32_MAX + 1 : tilesR * tilesC)
                              : cdiv(K * nbR, kBlock);
    if (grid > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    const int bits = fmt == FP8Q_MX_E2M1 ? 4 : (fp6 ? 6 : 8);
    MxthArgs ha = {};
    MxtArgs &a = ha.t;
    a.codes_t = codes_t;
    a.scales_t = scales_t;
    a.R = R;
    a.K = K;
    a.nbR = nbR;
    a.nbK = cdiv(K, kMxBlock);
    a.pitch_t = R * bits / 8;
    a.tilesC = tilesC;
    a.ceil_rule = rounding == FP8Q_MX_CEIL;
    a.gran = route.code_store_bytes;
    if (sr) a.sr = *sr;
    ha.mask = mask;
    const dim3 g((unsigned)grid), b(kBlock);
    auto run = [&](auto fc, auto in, auto outp, auto sr_on) {
        constexpr int F = decltype(fc)::value;
        constexpr bool SR = decltype(sr_on)::value;
        typedef decltype(in) IN;
        typedef decltype(outp) OUT;
        if (!tile) hipLaunchKernelGGL((k_mxth_plain<QUANT, F, IN, OUT, SR>), g, b, 0, st, x, y, ha);
        else if (route.nontemporal) hipLaunchKernelGGL((k_mxth<QUANT, F, IN, OUT, true, SR>), g, b, 0, st, x, y, ha);
        else hipLaunchKernelGGL((k_mxth<QUANT, F, IN, OUT, false, SR>), g, b, 0, st, x, y, ha);
    };
    auto go = [&](auto fc, auto in, auto outp) {
        if (sr) run(fc, in, outp, std::true_type{});
        else run(fc, in, outp, std::false_type{});
    };
    dispatch<FP8Q_MX_E4M3FN, FP8Q_MX_E5M2, FP8Q_MX_E2M3, FP8Q_MX_E3M2, FP8Q_MX_E2M1>(fmt, [&](auto fc) {
        value_io(x_type, [&](auto in) {
            if constexpr (!QUANT) {
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

int fp8q_mxh_encode_t_f32(const float *x, uint8_t *codes_t, uint8_t *scales_t, int64_t R, int64_t K, int fmt, int rounding,
                          uint32_t sign_mask, int sr, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    MxSr s;
    const MxSr *use;
    if (int rc = had_sr_args(sr, seed, offset, &s, &use)) return rc;
    return mxth_launch<false>(x, nullptr, codes_t, scales_t, FP8Q_DT_F32, -1, R, K, fmt, rounding, sign_mask,
                              (hipStream_t)stream, use);
}

int fp8q_mxh_encode_t_h16(const void *x, uint8_t *codes_t, uint8_t *scales_t, int x_type, int64_t R, int64_t K, int fmt,
                          int rounding, uint32_t sign_mask, int sr, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    MxSr s;
    const MxSr *use;
    if (int rc = had_sr_args(sr, seed, offset, &s, &use)) return rc;
    return mxth_launch<false>(x, nullptr, codes_t, scales_t, x_type, -1, R, K, fmt, rounding, sign_mask, (hipStream_t)stream,
                              use);
}

int fp8q_mxh_quantize_t_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, uint32_t sign_mask, int sr,
                            uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    MxSr s;
    const MxSr *use;
    if (int rc = had_sr_args(sr, seed, offset, &s, &use)) return rc;
    return mxth_launch<true>(x, y, nullptr, nullptr, FP8Q_DT_F32, FP8Q_DT_F32, R, K, fmt, rounding, sign_mask,
                             (hipStream_t)stream, use);
}

int fp8q_mxh_quantize_t_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                            uint32_t sign_mask, int sr, uint64_t seed, uint64_t offset, fp8q_stream_t stream)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    MxSr s;
    const MxSr *use;
    if (int rc = had_sr_args(sr, seed, offset, &s, &use)) return rc;
    return mxth_launch<true>(x, y, nullptr, nullptr, x_type, y_type, R, K, fmt, rounding, sign_mask, (hipStream_t)stream, use);
}

}  // extern "C"
