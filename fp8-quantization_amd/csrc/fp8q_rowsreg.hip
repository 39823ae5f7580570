// fp8q_rowsreg.hip -- k_rows_reg and its launcher: its 112 instantiations (4 lane counts x 7 slot counts x NT x QUANT)
// compile longer than the rest of the family together (profiles/quant_split_build.txt), hence a unit of their own.
#include "fp8q_rows.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Fused K2+K5+K1 for rows of 257..8192 elements (a multiple of 4, 16-byte aligned): the row stays in
// REGISTERS between the min/max pass and the quantize pass, so the tensor is read once (8 B/element of
// HBM traffic for real).  L lanes per row: 16 or 32 (16 / 8 rows per block), 64 (one wave per row) or 256
// (the whole block per row); the host picks the L whose lanes are best filled.  Rows are handed out grid-stride, so concurrently running blocks
// work on neighbouring rows -- the access pattern of a copy.  Per row: EPT x 16 B per lane in flight,
// wave (+ LDS) min/max reduction, the row's {s, 1/s} table written by its own lanes, quantize, store.
// ---------------------------------------------------------------------------------------------
template <int L, int EPT, bool NT, bool QUANT>
__global__ void __launch_bounds__(kBlock)
k_rows_reg(const float *__restrict__ x, float *__restrict__ y, int64_t C, int inner, float *row_min,
           float *row_max, float *maxval_out, QFmt f, FoldArgs fa)
{
    constexpr int RPB = kBlock / L;      // rows per block and step (L = lanes per row: 16, 32, 64 or 256)
    __shared__ float2 lut[RPB][kLutMax];
    __shared__ double ftab[kFastTabSize];
    __shared__ float s_mn[4], s_mx[4];
    __shared__ int s_nan[4];
    const int tid = threadIdx.x, sub = tid % L, rslot = tid / L, wave = tid >> 6;
    const int nvec = inner >> 2, rem = inner & 3;   // rem != 0 only for K2
    const float pmaxf = (float)f.pmax;
    if (QUANT) {
        for (int i = tid; i < kFastTabSize; i += kBlock) ftab[i] = kFastTab[i];
        __syncthreads();
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < C; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t row = r0 + rslot;
        const bool valid = row < C;
        const float *xr = x + (valid ? row : 0) * inner;
        vf4 v[EPT];
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            v[k] = vf4{0.0f, 0.0f, 0.0f, 0.0f};   // a group beyond the row: quantizes to 0 on the fast path, never stored
            const int idx = k * L + sub;
            if (valid && idx < nvec) {
                v[k] = ld16u<NT>(xr + 4 * idx);   // rows may start at any 4-byte phase (K2); one dwordx4 either way
            } else if (!QUANT && valid && idx == nvec && rem) {   // K2 only: the row's last 1..3 elements
                v[k].x = xr[4 * idx];
                if (rem > 1) v[k].y = xr[4 * idx + 1];
                if (rem > 2) v[k].z = xr[4 * idx + 2];
            }
        }
        MinMax m;
        mm_init(m);
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int idx = k * L + sub;
            if (valid && idx < nvec) {
                mm_acc(m, v[k].x);
                mm_acc(m, v[k].y);
                mm_acc(m, v[k].z);
                mm_acc(m, v[k].w);
            } else if (!QUANT && valid && idx == nvec && rem) {
                mm_acc(m, v[k].x);
                if (rem > 1) mm_acc(m, v[k].y);
                if (rem > 2) mm_acc(m, v[k].z);
            }
        }
#pragma unroll
        for (int off = (L < 64 ? L : 64) >> 1; off >= 1; off >>= 1) {
            m.mn = fminf(m.mn, __shfl_xor(m.mn, off, 64));
            m.mx = fmaxf(m.mx, __shfl_xor(m.mx, off, 64));
            m.nan |= __shfl_xor(m.nan, off, 64);
        }
        if (L == 256) {
            if ((tid & 63) == 0) {
                s_mn[wave] = m.mn;
                s_mx[wave] = m.mx;
                s_nan[wave] = m.nan;
            }
            __syncthreads();
            m.mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
            m.mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
            m.nan = s_nan[0] | s_nan[1] | s_nan[2] | s_nan[3];
        }
        if (m.nan) m.mn = m.mx = __builtin_nanf("");
        if (!QUANT) {   // K2: fold into the running estimate and go on (no tables, no stores)
            if (valid && sub == 0) fold_store(m.mn, m.mx, row, row_min, row_max, maxval_out, fa);
            if (L == 256) __syncthreads();   // s_mn / s_mx are rewritten by the next step
            continue;
        }
        const float mv = fabsf(tmax(fabsf(m.mn), m.mx));   // fp8_quantizer.py:236
        if (valid && sub == 0) {
            if (row_min) row_min[row] = m.mn;
            if (row_max) row_max[row] = m.mx;
            if (maxval_out) maxval_out[row] = mv;
        }
        const Chan c = make_chan_fast(mv, f, ftab);
        for (int p = sub; p <= f.pmax; p += L) lut[rslot][p] = lut_entry(c, p, f.M);
        __syncthreads();
        {
            // one branch for all groups of the lane (missing groups hold zeros: no rare-case work)
            const ChanLite cl = lite(c);
            vf4 *yv = reinterpret_cast<vf4 *>(y + (valid ? row : 0) * inner);
            float e[EPT * 4];
#pragma unroll
            for (int k = 0; k < EPT; ++k) {
                e[4 * k] = v[k].x;
                e[4 * k + 1] = v[k].y;
                e[4 * k + 2] = v[k].z;
                e[4 * k + 3] = v[k].w;
            }
            quant_group<EPT * 4, false>(e, cl, lut[rslot], pmaxf, f.qthr);   // fused: a NaN makes the row's range NaN -> all-exact
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                if (valid && k * L + sub < nvec)
                    st16<NT>(yv + k * L + sub, vf4{e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3]});
        }
        __syncthreads();   // the tables are rewritten by the next step
    }
}

}  // namespace

// k_rows_reg for [C, inner] if the rows suit it (128..8192 elements, a multiple of 4, 16-byte aligned, lanes well
// filled); kNotFlat otherwise.  quant: fused min/max + quantize; else K2 (min/max + fold).
int fp8q_launch_rows_reg(bool quant, const float *x, float *y, int64_t C, int64_t inner, float *row_min, float *row_max,
                    float *maxval_out, const QFmt &f, const FoldArgs &fa, hipStream_t st, fp8q_rows_route_info *rec)
{
    static const int reg_env = env_int("FP8Q_FUSED_REG", 1);   // FP8Q_FUSED_REG=0: never (A/B against the row-tiled kernels)
    if (!reg_env || inner > 8192) return kNotFlat;
    if (quant && (inner < 128 || (inner & 3) != 0 || (((uintptr_t)x | (uintptr_t)y) & 15) != 0)) return kNotFlat;
    if (!quant && (inner < 68 || ((uintptr_t)x & 3) != 0)) return kNotFlat;   // K2 reads rows at any 4-byte phase
    // lanes per row and 16-byte slots per lane (EPT, instantiated for 2..8): the best-filled combination --
    // rows of 576 elements run 8 per block on 32 lanes x 5 slots (90 % filled)
    int reg_lanes = 0, reg_ept = 0;
    const int64_t nvec = (inner + 3) >> 2;
    int64_t best = 0;
    for (int lanes : {16, 32, 64, 256}) {
        const int64_t ept = cdiv(nvec, lanes);
        if (ept < 2 || ept > 8) continue;
        const int64_t fill = nvec * 1000 / (ept * lanes);
        if (fill > best) {
            best = fill;
            reg_lanes = lanes;
            reg_ept = (int)ept;
        }
    }
    if (best < 800) return kNotFlat;   // (147-element rows, 77 % filled: 4.8 TB/s here against 5.4 in k_rows_direct<2>)
    const bool nt = C * inner * 4 >= kNtBytes;
    const int64_t steps = cdiv(C, kBlock / reg_lanes);
    const int64_t grid = balanced_blocks(steps, 65536);
    const auto fill = [&](fp8q_rows_route_info &r) {
        r.kernel = FP8Q_ROWS_K_ROWS_REG;
        r.nontemporal = nt;
        r.lanes = reg_lanes;
        r.slots = reg_ept;
        r.grid_x = grid;
        r.grid_y = 1;
    };
    return rows_emit(rec, fill, [&] {
        dispatch<16, 32, 64, 256>(reg_lanes, [&](auto LN) {
            dispatch<2, 3, 4, 5, 6, 7, 8>(reg_ept, [&](auto E) {
                dispatch<true, false>(nt, [&](auto NT) {
                    dispatch<true, false>(quant, [&](auto QUANT) {
                        hipLaunchKernelGGL((k_rows_reg<LN(), E(), NT(), QUANT()>), dim3((unsigned)grid), dim3(kBlock), 0, st, x, y, C,
                                           (int)inner, row_min, row_max, maxval_out, f, fa);
                    });
                });
            });
        });
    });
}
