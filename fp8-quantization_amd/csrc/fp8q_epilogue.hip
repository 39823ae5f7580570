// fp8q_epilogue.hip -- N2: eval-BN + residual + ReLU/ReLU6 fused with the per-tensor activation quantizer, and its range twin.
#include "fp8q_common.h"
#include "fp8q_affine.h"

namespace {

__global__ void __launch_bounds__(kBlock)
k_bn_fold(const float *__restrict__ mean, const float *__restrict__ invstd, const float *__restrict__ gamma,
          const float *__restrict__ beta, int64_t C, float2 *__restrict__ ab)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c < C) ab[c] = bn_ab(mean, invstd, gamma, beta, (uint32_t)c, 1);
}

// {channel constants, table} of one per-tensor quantizer, laid out as k_affine_act_small copies them: float4 {maxval, lo,
// bias, pthr} followed by float2 {s_p, 1 / s_p}, p = 0 .. pmax
__global__ void __launch_bounds__(kBlock)
k_quantizer_prepare(const float *__restrict__ maxval, QFmt f, float4 *__restrict__ prep)
{
    const Chan cfull = make_chan(maxval[0], f);
    if (threadIdx.x == 0) prep[0] = make_float4(cfull.maxv, cfull.minv, cfull.bias, cfull.pthr);
    for (int i = threadIdx.x; i <= f.pmax; i += kBlock) reinterpret_cast<float2 *>(prep + 1)[i] = lut_entry(cfull, i, f.M);
}

// blockIdx.y = image n; blockIdx.x strides over the image's C*HW elements in aligned 16 KiB pieces
// (one piece per block when the grid allows it: measured 6.1-6.3 TB/s against 5.0 for a persistent
// grid of 2048 blocks).  Eval-mode batch norm exactly as ATen's CPU kernel evaluates it (probed:
// bit-identical on 100 % of elements): alpha = invstd * gamma, beta' = fma(-mean, alpha, beta),
// out = fma(x, alpha, beta'); {alpha, beta'} of the planes a piece overlaps are staged in LDS per
// step, the plane of a 16-byte group comes from one 32-bit magic division of its piece-local offset.
template <bool NT, int U>
__global__ void __launch_bounds__(kBlock)
k_affine_act(const float *__restrict__ x, const float *__restrict__ res, float *__restrict__ y,
             const float *__restrict__ mean, const float *__restrict__ invstd,
             const float *__restrict__ gamma, const float *__restrict__ beta,
             const float *__restrict__ maxval, QFmt f, AffineArgs a)
{
    __shared__ float2 lut[kLutMax];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *cst = reinterpret_cast<float2 *>(smem);   // [cpp] {alpha, beta'} (has_bn only)
    const int tid = threadIdx.x;
    ChanLite c = {};
    if (!a.passthrough) {
        const Chan cfull = make_chan(maxval[0], f);
        for (int i = tid; i <= f.pmax; i += kBlock) lut[i] = lut_entry(cfull, i, f.M);
        c = lite(cfull);
    }
    const float pmaxf = (float)f.pmax;
    const int64_t base0 = (int64_t)blockIdx.y * a.image;
    const int nvec = (int)(a.image >> 2);
    const vf4 *xv = reinterpret_cast<const vf4 *>(x + base0);
    const vf4 *rv = reinterpret_cast<const vf4 *>(res + (a.has_res ? base0 : 0));
    vf4 *yv = reinterpret_cast<vf4 *>(y + base0);
    const uint32_t HW = (uint32_t)a.HW;
    // planes of >= 4096 elements: a piece overlaps at most two, whose constants every thread keeps in registers
    // (uniform addresses: scalar loads) -- no LDS staging and no barrier per step, which is what separates the BN
    // variant from the plain one on the large early layers (75 -> 70 us at [64,64,112,112]; the same with up to
    // four planes in registers, for 56x56 planes, was measured and rejected: 94 us)
    const bool direct = affine_direct(a);
    __syncthreads();       // lut is complete
    for (int base = blockIdx.x * (kBlock * U); base < nvec; base += gridDim.x * (kBlock * U)) {
        float2 p0, p1;
        const uint32_t phase = affine_step_planes(base, direct, a, p0, p1, cst, [&](uint32_t ch) {
            return bn_ab(mean, invstd, gamma, beta, ch, a.has_bn);
        });
        auto transform = [&](int q, float (&e)[4], const vf4 &r) {   // q: piece-local group index
            const float rr[4] = {r.x, r.y, r.z, r.w};
            if (direct) {
                const uint32_t o = phase + 4u * (uint32_t)q;
                const bool hi = o >= HW;                    // second plane of the piece
                affine_walk(e, rr, hi ? o - HW : o, HW, hi ? p1 : p0, a, [&] { return p1; });
            } else if (a.has_bn) {
                const uint32_t o = phase + 4u * (uint32_t)q;
                uint32_t lch = affine_local_plane(o, a);
                affine_walk(e, rr, o - lch * HW, HW, cst[lch], a, [&] { return cst[++lch]; });
            } else {
                affine_plain(e, rr, a);
            }
        };
        if (base + kBlock * U <= nvec) {   // whole piece: unpredicated loads, one branch for all its elements
            vf4 vx[U], vr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) vx[u] = ld16<NT>(xv + base + u * kBlock + tid);
#pragma unroll
            for (int u = 0; u < U; ++u)
                vr[u] = a.has_res ? ld16<NT>(rv + base + u * kBlock + tid) : vf4{0.0f, 0.0f, 0.0f, 0.0f};
            float e[U * 4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float t[4] = {vx[u].x, vx[u].y, vx[u].z, vx[u].w};
                transform(u * kBlock + tid, t, vr[u]);
                e[4 * u] = t[0];
                e[4 * u + 1] = t[1];
                e[4 * u + 2] = t[2];
                e[4 * u + 3] = t[3];
            }
            if (!a.passthrough) quant_group<U * 4>(e, c, lut, pmaxf, f.qthr);
#pragma unroll
            for (int u = 0; u < U; ++u)
                st16<NT>(yv + base + u * kBlock + tid, vf4{e[4 * u], e[4 * u + 1], e[4 * u + 2], e[4 * u + 3]});
        } else {
            for (int u = 0; u < U; ++u) {
                const int j = base + u * kBlock + tid;
                if (j >= nvec) break;
                const vf4 v = xv[j];
                const vf4 r = a.has_res ? ld16<NT>(rv + j) : vf4{0.0f, 0.0f, 0.0f, 0.0f};
                float e[4] = {v.x, v.y, v.z, v.w};
                transform(u * kBlock + tid, e, r);
                if (!a.passthrough) quant_group<4>(e, c, lut, pmaxf, f.qthr);
                st16<NT>(yv + j, vf4{e[0], e[1], e[2], e[3]});
            }
        }
    }
}

// Small (cache-sized) activations: the launch is latency-bound -- what counts is the length of the dependent chain from
// block start to the first store, not bandwidth.  k_affine_act's chain is {maxval -> channel constants -> table} ->
// barrier -> {BN vectors -> LDS} -> barrier -> {x} -> arithmetic -> store: three memory round trips behind each other
// where the plain K1 has two.  Here a lane handles ONE 16-byte group per step and fetches the BN vectors of its own
// plane(s) straight from global memory (L2 hits: <= 20 KB per model layer) next to x itself, so x, residual and the BN
// vectors are one round trip, issued BEFORE the table is built so that the table's arithmetic hides it (issuing it behind
// the table, as the first version of this kernel did, was slower and is no longer built).
// rocprofv3 kernel durations at batch 64 (round 3's staged kernel -> this one): [64,160,7,7] 5.4 -> 4.4 us, [64,96,14,14]
// 6.7 -> 5.3, [64,576,7,7] 6.7 -> 5.5, [64,384,14,14] 12.2 -> 9.5, [64,144,28,28] 16.0 -> 13.1 (plain K1 on the same
// tensors: 3.9 / 5.1 / 5.1 / 7.3 / 10.4); it wins up to the nontemporal threshold ([64,192,28,28] 19.7 -> 14.8 us,
// [64,64,56,56] 21.2 -> 18.5) and loses beyond it, where the staged kernel's LDS constants cost less than eight extra
// dword loads per group ([64,96,56,56] 31.3 vs 35.6 us with NT = true, U = 4) -- so it serves every tensor below 64 MiB.
// Measured and rejected on top of it: 2 or 4 groups per lane and step (U = 2: +8...12 %, U = 4: +15...35 % time),
// nontemporal accesses below 64 MiB (+10 %), grids of 1024...16384 blocks (2048...4096 equal, the rest worse), requesting
// the next step's group before the arithmetic of the current one (no change).  With the folded BN vector (has_bn == 2:
// two 8-byte loads per group instead of eight 4-byte ones) another 5-8 %: [64,64,56,56] 19.9 -> 18.5 us (K1: 17.9).
__global__ void __launch_bounds__(kBlock)
k_affine_act_small(const float *__restrict__ x, const float *__restrict__ res, float *__restrict__ y,
                   const float *__restrict__ mean, const float *__restrict__ invstd, const float *__restrict__ gamma,
                   const float *__restrict__ beta, const float *__restrict__ maxval, QFmt f, AffineArgs a,
                   const float4 *__restrict__ prep)
{
    __shared__ float2 lut[kLutMax];
    const int tid = threadIdx.x;
    const int64_t base0 = (int64_t)blockIdx.y * a.image;
    const int nvec = (int)(a.image >> 2);
    const vf4 *xv = reinterpret_cast<const vf4 *>(x + base0);
    const vf4 *rv = reinterpret_cast<const vf4 *>(res + (a.has_res ? base0 : 0));
    vf4 *yv = reinterpret_cast<vf4 *>(y + base0);
    const int step = gridDim.x * kBlock;
    int base = blockIdx.x * kBlock;
    AffineGrp g;
    if (base + tid < nvec) affine_fetch(g, xv, rv, base + tid, mean, invstd, gamma, beta, a.has_bn, a);
    // The quantizer's channel constants and {s, 1/s} table: rebuilt from maxval (a load, ~50 dependent double-precision
    // operations, the table entries) -- or, with fixed ranges, copied from the block fp8q_quantizer_prepare_f32 wrote once:
    // the same numbers, one 8-byte load per entry, 0.5-1 us less on the critical path of a 4-10 us launch.
    ChanLite c = {};
    if (a.passthrough) {
    } else if (prep) {
        const float4 h = prep[0];
        c.maxv = h.x;
        c.minv = h.y;
        c.bias = h.z;
        c.pthr = h.w;
        for (int i = tid; i <= f.pmax; i += kBlock) lut[i] = reinterpret_cast<const float2 *>(prep + 1)[i];
    } else {
        const Chan cfull = make_chan(maxval[0], f);
        for (int i = tid; i <= f.pmax; i += kBlock) lut[i] = lut_entry(cfull, i, f.M);
        c = lite(cfull);
    }
    const float pmaxf = (float)f.pmax;
    __syncthreads();
    bool first = true;   // its group is already here
    for (; base < nvec; base += step) {
        const int j = base + tid;
        if (j < nvec && !first) affine_fetch(g, xv, rv, j, mean, invstd, gamma, beta, a.has_bn, a);
        first = false;
        if (j >= nvec) break;
        float e[4];
        affine_apply(g, e, a);
        if (!a.passthrough) quant_group<4>(e, c, lut, pmaxf, f.qthr);
        yv[j] = vf4{e[0], e[1], e[2], e[3]};
    }
}

// Calibration twin of k_affine_act: min / max of act(bn(x) + residual); the block that finishes last folds all blocks'
// partials into the running estimate (block_minmax_fold: one launch).  Read-only, so the
// trade-offs differ from the quantizing kernel: a persistent grid of <= 2048 blocks with 4 KiB steps, plain
// loads and the constants straight from global measured best (36 us at [64,64,112,112]; 16 KiB steps, LDS-staged
// constants, nontemporal loads or one piece per block: 42-55 us).
// STORE: the transformed tensor t is also written (fp8q_affine_act_minmax_linspace_f32: the first calibration batch of an MSE
// estimator behind a BN + activation needs t itself, its abs-max and the search grid of that maximum -- one pass instead of
// torch's batch_norm + activation + this library's abs-max pass).
template <bool STORE>
__global__ void __launch_bounds__(kBlock)
k_affine_minmax(const float *__restrict__ x, const float *__restrict__ res, const float *__restrict__ mean,
                const float *__restrict__ invstd, const float *__restrict__ gamma,
                const float *__restrict__ beta, AffineArgs a, int64_t N, unsigned long long *slots, int nparts,
                unsigned tag, float *cur_min, float *cur_max, float *maxval_out, FoldArgs fa, float *__restrict__ t_out)
{
    const int nby = nparts / (int)gridDim.x;   // block rows that stream; one more row holds the reducer (nparts > 1)
    if ((int)blockIdx.y == nby) {
        if (blockIdx.x == 0) block_minmax_collect(slots, nparts, tag, 0, cur_min, cur_max, maxval_out, fa);
        return;
    }
    const int tid = threadIdx.x;
    MinMax mm;
    mm_init(mm);
    const int nvec = (int)(a.image >> 2);
    const uint32_t HW = (uint32_t)a.HW;
    for (int64_t img = blockIdx.y; img < N; img += nby) {   // more than 65535 images: several per block row
    const int64_t base = img * a.image;
    const vf4 *xv = reinterpret_cast<const vf4 *>(x + base);
    const vf4 *rv = reinterpret_cast<const vf4 *>(res + (a.has_res ? base : 0));
    for (int j = blockIdx.x * kBlock + tid; j < nvec; j += gridDim.x * kBlock) {
        const vf4 v = xv[j];
        vf4 r = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.has_res) r = rv[j];
        float e[4] = {v.x, v.y, v.z, v.w};
        const float rr[4] = {r.x, r.y, r.z, r.w};
        if (a.has_bn) {
            const uint32_t i0 = (uint32_t)j * 4u;
            uint32_t ch = (uint32_t)(((uint64_t)i0 * a.magic48) >> 48);      // plane == channel
            affine_walk(e, rr, i0 - ch * HW, HW, bn_ab(mean, invstd, gamma, beta, ch, a.has_bn), a,
                        [&] { return bn_ab(mean, invstd, gamma, beta, ++ch, a.has_bn); });
        } else {
            affine_plain(e, rr, a);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) mm_acc(mm, e[q]);
        if (STORE) reinterpret_cast<vf4 *>(t_out + base)[j] = vf4{e[0], e[1], e[2], e[3]};
    }
    }
    block_minmax_publish(mm, slots, (int)(blockIdx.y * gridDim.x + blockIdx.x), nparts, tag, 0, cur_min, cur_max,
                         maxval_out, fa);
}

}  // namespace

extern "C" {

// k_affine_minmax<true> (the epilogue that also WRITES t: first calibration batch of an MSE estimator): the read-only twin's
// persistent grid of <= 2048 blocks with four 16-byte groups per thread and step leaves a small activation on a fraction of
// the chip ([64,160,7,7]: 128 blocks, 10.5 us against 4.9 for the plain epilogue on the same tensor) -- a group per thread
// while the grid stays below FP8Q_EPI_MM_GRID (2048) blocks (more blocks = more partials for the reducer to poll: 4096 and up were slower on
// every shape; four groups per thread and step requested together, or nontemporal accesses beyond the caches: no gain / slower).
static void affine_grid_store(int64_t N, const AffineArgs &a, int64_t *bx, int64_t *by)
{
    static const int64_t cap_env = [] {
        const char *e = getenv("FP8Q_EPI_MM_GRID");
        const long v = e ? atol(e) : 0;
        return (int64_t)(v > 0 ? v : 2048);
    }();
    *by = N < 65534 ? N : 65534;
    const int64_t nvec = a.image >> 2;
    const int64_t pieces = cdiv(nvec, kBlock);
    *bx = balanced_blocks(pieces, cap_env / *by > 0 ? cap_env / *by : 1);
}

int fp8q_bn_fold_f32(const float *mean, const float *invstd, const float *gamma, const float *beta, int64_t C,
                     float *alpha_beta, fp8q_stream_t stream)
{
    if (C < 0 || (C > 0 && (!mean || !invstd || !gamma || !beta || !alpha_beta || ((uintptr_t)alpha_beta & 7)))) return FP8Q_EINVAL;
    if (C == 0) return FP8Q_OK;
    hipLaunchKernelGGL(k_bn_fold, dim3((unsigned)cdiv(C, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, mean, invstd, gamma,
                       beta, C, reinterpret_cast<float2 *>(alpha_beta));
    return launch_rc();
}

static int affine_quantize_impl(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW,
                                const float *mean, const float *invstd, const float *gamma, const float *beta, int has_bn,
                                int act, const float *maxval, const float *prep, float mbits, int n_bits, int sign_bits,
                                fp8q_stream_t stream, int passthrough = 0);

int fp8q_affine_act_quantize_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C,
                                 int64_t HW, const float *mean, const float *invstd, const float *gamma,
                                 const float *beta, int act, const float *maxval, float mbits, int n_bits,
                                 int sign_bits, fp8q_stream_t stream)
{
    const int has_bn = mean != nullptr;
    if (has_bn && (!invstd || !gamma || !beta)) return FP8Q_EINVAL;
    return affine_quantize_impl(x, residual, y, N, C, HW, mean, invstd, gamma, beta, has_bn, act, maxval, nullptr, mbits, n_bits,
                                sign_bits, stream);
}

int fp8q_quantizer_prepare_f32(const float *maxval, float mbits, int n_bits, int sign_bits, float *prep, fp8q_stream_t stream)
{
    if (!maxval || !prep || ((uintptr_t)prep & 15)) return FP8Q_EINVAL;
    QFmt f;
    if (int rc = make_fmt(mbits, n_bits, sign_bits, &f)) return rc;
    hipLaunchKernelGGL(k_quantizer_prepare, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, maxval, f, reinterpret_cast<float4 *>(prep));
    return launch_rc();
}

int fp8q_affine_act_quantize_ab_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW,
                                    const float *alpha_beta, int act, const float *maxval, const float *prep, float mbits,
                                    int n_bits, int sign_bits, fp8q_stream_t stream)
{
    if (((uintptr_t)alpha_beta & 7) || ((uintptr_t)prep & 15)) return FP8Q_EINVAL;
    return affine_quantize_impl(x, residual, y, N, C, HW, alpha_beta, nullptr, nullptr, nullptr, alpha_beta ? 2 : 0, act, maxval,
                                prep, mbits, n_bits, sign_bits, stream);
}

int fp8q_affine_act_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW, const float *alpha_beta,
                        int act, fp8q_stream_t stream)
{
    if ((uintptr_t)alpha_beta & 7) return FP8Q_EINVAL;
    // the quantizing kernels with the quantizer switched off: same geometry, same BN arithmetic (what the quantizer will see)
    return affine_quantize_impl(x, residual, y, N, C, HW, alpha_beta, nullptr, nullptr, nullptr, alpha_beta ? 2 : 0, act, nullptr, nullptr,
                                3.0f, 8, 1, stream, 1);
}

static int affine_quantize_impl(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW,
                                const float *mean, const float *invstd, const float *gamma, const float *beta, int has_bn,
                                int act, const float *maxval, const float *prep, float mbits, int n_bits, int sign_bits,
                                fp8q_stream_t stream, int passthrough)
{
    AffineArgs a;
    if (int rc = affine_args(N, C, HW, act, has_bn, residual != nullptr, &a)) return rc;
    a.passthrough = passthrough != 0;
    QFmt f;
    if (int rc = make_fmt(mbits, n_bits, sign_bits, &f)) return rc;
    if (N == 0) return FP8Q_OK;
    if (!x || !y || (!maxval && !passthrough)) return FP8Q_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)residual) & 15) return FP8Q_EINVAL;
    affine_dispatch(N, a, true, [&](AffineKernel kind, dim3 g, size_t shm, int64_t n0) {
        const float *xp = x + n0 * a.image, *rp = residual ? residual + n0 * a.image : nullptr;
        float *yp = y + n0 * a.image;
        const hipStream_t st = (hipStream_t)stream;
        if (kind == AffineKernel::Small)
            hipLaunchKernelGGL(k_affine_act_small, g, dim3(kBlock), 0, st, xp, rp, yp, mean, invstd, gamma, beta, maxval, f, a,
                               reinterpret_cast<const float4 *>(prep));
        else
            hipLaunchKernelGGL((kind == AffineKernel::StagedNt  ? k_affine_act<true, 4>
                                : kind == AffineKernel::Staged1 ? k_affine_act<false, 1> : k_affine_act<false, 4>),
                               g, dim3(kBlock), shm, st, xp, rp, yp, mean, invstd, gamma, beta, maxval, f, a);
    });
    return launch_rc();
}

// What affine_quantize_impl would launch for this shape: its own affine_args + affine_dispatch with a callback that records
// instead of launching.  Host arithmetic only.
static_assert((int)AffineKernel::StagedNt == FP8Q_AFFINE_STAGED_NT && (int)AffineKernel::Small == FP8Q_AFFINE_SMALL &&
              (int)AffineKernel::Staged1 == FP8Q_AFFINE_STAGED1 && (int)AffineKernel::Staged4 == FP8Q_AFFINE_STAGED4,
              "fp8q_affine_route_info.kernel is AffineKernel's value");

int fp8q_affine_act_route(int64_t N, int64_t C, int64_t HW, int has_bn, fp8q_affine_route_info *info)
{
    if (!info || has_bn < 0 || has_bn > 2) return FP8Q_EINVAL;
    AffineArgs a;
    if (int rc = affine_args(N, C, HW, 0, has_bn, false, &a)) return rc;
    fp8q_affine_route_info r = {};
    r.kernel = -1;      // N == 0: nothing is launched
    r.cpp = a.cpp;
    affine_dispatch(N, a, true, [&](AffineKernel kind, dim3 g, size_t, int64_t) {
        if (r.launches++ == 0) {
            r.kernel = (int)kind;
            r.direct = kind != AffineKernel::Small && affine_direct(a);
            r.grid_x = g.x;
            r.grid_y = g.y;
        }
    });
    *info = r;
    return FP8Q_OK;
}

size_t fp8q_affine_act_minmax_workspace_bytes(int64_t N, int64_t C, int64_t HW)
{
    AffineArgs a;
    if (N <= 0 || affine_args(N, C, HW, 0, false, false, &a) != FP8Q_OK) return 16;
    int64_t bx, by, sx, sy;
    affine_grid(N, a, false, &bx, &by);
    affine_grid_store(N, a, &sx, &sy);           // (the variant that writes t has its own grid: the larger of the two)
    const int64_t parts = bx * by > sx * sy ? bx * by : sx * sy;
    return kMinmaxWsHeader + (size_t)parts * 2 * sizeof(unsigned long long);   // header + two tagged granules per streaming block
}

static int affine_minmax_impl(const float *x, const float *residual, int64_t N, int64_t C, int64_t HW,
                              const float *mean, const float *invstd, const float *gamma, const float *beta,
                              int act, float *cur_min, float *cur_max, float *maxval_out, float *packed, int fold_mode,
                              double momentum, int first, void *ws, size_t ws_bytes, fp8q_stream_t stream,
                              int has_bn = -1, float *t_out = nullptr, float *lin_grid = nullptr, int lin_steps = 0,
                              double lin_lo = 0.0, double lin_hi = 0.0)
{
    if (has_bn < 0) has_bn = mean != nullptr;
    if (has_bn == 1 && (!invstd || !gamma || !beta)) return FP8Q_EINVAL;
    AffineArgs a;
    if (int rc = affine_args(N, C, HW, act, has_bn, residual != nullptr, &a)) return rc;
    if (N <= 0 || !x || !cur_min || !cur_max || fold_mode < 0 || fold_mode > 2) return FP8Q_EINVAL;
    if (!ws || ws_bytes < fp8q_affine_act_minmax_workspace_bytes(N, C, HW) || ((uintptr_t)ws & 7)) return FP8Q_EWORKSPACE;
    if ((((uintptr_t)x | (uintptr_t)residual) & 15) || ((uintptr_t)packed & 15)) return FP8Q_EINVAL;
    {
        static const bool debug_ws = env_int("FP8Q_DEBUG_WS", 0) != 0;
        if (debug_ws)
            if (int rc = fp8q_minmax_workspace_check(ws, fp8q_affine_act_minmax_workspace_bytes(N, C, HW), 0, stream)) return rc;
    }
    int64_t bx, by;
    if (t_out)
        affine_grid_store(N, a, &bx, &by);
    else
        affine_grid(N, a, false, &bx, &by);
    hipStream_t st = (hipStream_t)stream;
    FoldArgs fa;
    fa.mode = fold_mode;
    fa.first = first != 0;
    fa.om = (float)(1.0 - momentum);
    fa.mo = (float)momentum;
    fa.packed = packed;
    fa.status = (unsigned *)ws;
    fa.lin_grid = lin_grid;
    fa.lin_steps = lin_steps;
    fa.lin_C = 1;
    fa.lin_lo = lin_lo;
    fa.lin_hi = lin_hi;
    fold_debug_env(fa);
    const int nparts = (int)(bx * by);
    // one more block row for the reducer when there is more than one streaming block (by <= 65535 - 1: affine_grid)
    if (t_out)
        hipLaunchKernelGGL(k_affine_minmax<true>, dim3((unsigned)bx, (unsigned)(nparts > 1 ? by + 1 : by)), dim3(kBlock), 0, st, x,
                           residual, mean, invstd, gamma, beta, a, N, (unsigned long long *)((char *)ws + kMinmaxWsHeader), nparts,
                           next_minmax_tag(), cur_min, cur_max, maxval_out, fa, t_out);
    else
        hipLaunchKernelGGL(k_affine_minmax<false>, dim3((unsigned)bx, (unsigned)(nparts > 1 ? by + 1 : by)), dim3(kBlock), 0, st, x,
                           residual, mean, invstd, gamma, beta, a, N, (unsigned long long *)((char *)ws + kMinmaxWsHeader), nparts,
                           next_minmax_tag(), cur_min, cur_max, maxval_out, fa, nullptr);
    return launch_rc();
}

int fp8q_affine_act_minmax_f32(const float *x, const float *residual, int64_t N, int64_t C, int64_t HW,
                               const float *mean, const float *invstd, const float *gamma, const float *beta,
                               int act, float *cur_min, float *cur_max, float *maxval_out, int fold_mode,
                               double momentum, int first, void *ws, size_t ws_bytes, fp8q_stream_t stream)
{
    return affine_minmax_impl(x, residual, N, C, HW, mean, invstd, gamma, beta, act, cur_min, cur_max, maxval_out, nullptr,
                              fold_mode, momentum, first, ws, ws_bytes, stream);
}

int fp8q_affine_act_minmax_packed_f32(const float *x, const float *residual, int64_t N, int64_t C, int64_t HW,
                                      const float *mean, const float *invstd, const float *gamma, const float *beta,
                                      int act, float *cur_min, float *cur_max, float *maxval_out, float *packed,
                                      int fold_mode, double momentum, int first, void *ws, size_t ws_bytes,
                                      fp8q_stream_t stream)
{
    if (!packed) return FP8Q_EINVAL;
    return affine_minmax_impl(x, residual, N, C, HW, mean, invstd, gamma, beta, act, cur_min, cur_max, maxval_out, packed,
                              fold_mode, momentum, first, ws, ws_bytes, stream);
}

int fp8q_affine_act_minmax_linspace_f32(const float *x, const float *residual, float *t, int64_t N, int64_t C, int64_t HW,
                                        const float *alpha_beta, int act, float *cur_min, float *cur_max, float *maxval_out,
                                        float *grid, int n_cand, double lo_frac, double hi_frac, void *ws, size_t ws_bytes,
                                        fp8q_stream_t stream)
{
    if (!t || !grid || !maxval_out || n_cand < 2 || n_cand > (1 << 20) || ((uintptr_t)alpha_beta & 7) || ((uintptr_t)t & 15)) return FP8Q_EINVAL;
    return affine_minmax_impl(x, residual, N, C, HW, alpha_beta, nullptr, nullptr, nullptr, act, cur_min, cur_max, maxval_out, nullptr,
                              FP8Q_FOLD_CURRENT, 0.0, 1, ws, ws_bytes, stream, alpha_beta ? 2 : 0, t, grid, n_cand, lo_frac, hi_frac);
}

}  // extern "C"
