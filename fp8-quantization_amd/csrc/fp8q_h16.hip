// fp8q_h16.hip -- the half-precision lane: K1, row min/max (+ fold) and min/max + quantize on IEEE fp16 and bfloat16
// tensors (gfx950 only).  Element type selected at run time (x_type / y_type = FP8Q_DT_*, include/fp8q.h).
//
// Arithmetic contract:
//   - every input element is widened to fp32 EXACTLY: fp16 subnormals become normal fp32 numbers (v_cvt_f32_f16 with
//     fp16 denormals enabled, the HIP default), bf16 is the upper half of an fp32 word, so its subnormals become fp32
//     subnormals; nothing is flushed.  NaN stays NaN, infinities clamp like any value beyond maxval.
//   - from there the fp32 contract of fp8q_device.h:1-25 applies unchanged -- the same make_chan / lut_* / quant_group /
//     quant_exact / quant_direct code, fast path and exact path alike -- so the fp32 result is bit-identical to
//     oracle.c_quantize(widen(x), ...).  This is what the reference computes: maxval and the mantissa width are fp32
//     tensors, ATen's type promotion widens a half x and returns fp32 (fp8_quantizer.py:105-133).
//   - y_type == FP8Q_DT_F32 stores that result; y_type == x_type rounds it ONCE to the storage type, round to nearest
//     even, overflow to infinity (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32: what torch.Tensor.to(dtype) does).
//   - min/max: minimum and maximum of the widened row in fp32 with the NaN and signed-zero rules of fp8q_minmax_f32;
//     the running estimate, the fold and maxval_out are fp32 (fold_store, fp8q_common.h).
//
// Kernels:
//   k_h16_quant         K1 on the tensor as one flat range: the first (<= 7) elements up to x's 16-byte boundary and the
//                       last (<= 7) are scalars of block 0; the body is cut into chunks of 256 * U groups of 8 elements
//                       (one 16-byte load per lane and group, U in flight).  The {s, 1/s} tables of the rows overlapping
//                       the chunk are built in LDS while the loads fly.  A group that straddles a row border (rows of
//                       >= 8 elements: at most two rows per group) takes each element's constants and table from its own row.
//                       The output goes out as 16 bytes (half) or 2 x 16 bytes (fp32) per group at the alignment y
//                       happens to have: y need not share x's phase, and y == x (same type) is safe because a lane
//                       writes only the group it has read.
//   k_h16_quant_rows    K1 for what the chunk kernel does not take (per-channel rows shorter than 8 elements, rows so
//                       short that the tables of a chunk outgrow LDS): thread = row, no table (quant_direct).
//   k_h16_minmax_rows   K2 (+ fold, K5) for per-channel rows up to 2048 elements: 2^gs lanes per row, 16-byte loads of 8
//                       elements at the row's own 2-byte phase (neighbouring lanes neighbouring groups), shuffle reduction.
//   k_h16_minmax_part   K2/K3 for long rows: fp32's two-stage single-launch scheme (fp8q_common.h) with 8 elements
//                       per 16-byte load.
// HBM traffic per element: K1 6 B (fp32 out) or 4 B (half out); min/max 2 B; min/max + quantize: a 2 B scan, then K1.
#include "fp8q_common.h"
#include "fp8q_half.h"

namespace {

// quant_group<8> (fp8q_device.h) for a group whose elements b..7 belong to a second channel
__device__ __forceinline__ void quant_group_2rows(float (&v)[8], int b, const ChanLite &ca, const float2 *la, const ChanLite &cb,
                                                  const float2 *lb, float pmaxf, float qthr)
{
    float y[8];
    bool rk[8];
    bool any = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool nx = j >= b;
        ChanLite c;
        c.maxv = nx ? cb.maxv : ca.maxv;
        c.minv = nx ? cb.minv : ca.minv;
        c.bias = nx ? cb.bias : ca.bias;
        c.pthr = nx ? cb.pthr : ca.pthr;
        y[j] = quant_fast(v[j], c, nx ? lb : la, pmaxf, qthr, rk[j]);
        any |= rk[j];
    }
    if (__builtin_expect(any, 0)) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (rk[j]) {
                const bool nx = j >= b;
                y[j] = nx ? quant_exact(v[j], cb.maxv, cb.minv, cb.bias, lb, pmaxf) : quant_exact(v[j], ca.maxv, ca.minv, ca.bias, la, pmaxf);
            }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = y[j];
}

struct H16Args {
    int64_t n;         // elements of the tensor
    int64_t head;      // scalars in front of the 16-byte aligned body (<= 7)
    int64_t ng;        // 8-element groups of the body
    int64_t inner;     // row length (per channel), n otherwise
    uint32_t magic;    // o / inner for chunk-local offsets (rows shorter than a chunk)
    int lut_stride;    // pmax + 1
    int nc_max;        // rows a chunk can overlap: LDS entries
};

constexpr size_t kH16LdsBudget = 40 * 1024;   // tables of one chunk

template <class T, bool YF32, bool PC, int U, bool NT>
__global__ void __launch_bounds__(kBlock)
k_h16_quant(const uint16_t *x, void *y, const float *__restrict__ maxval, QFmt f, H16Args a)   // (y may be x: no __restrict__)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *chl = reinterpret_cast<float4 *>(smem);
    float2 *lut = reinterpret_cast<float2 *>(chl + a.nc_max);
    constexpr int CH = kBlock * 8 * U;
    const int tid = threadIdx.x;
    const float pmaxf = (float)f.pmax;

    // the body's loads first: the table build below hides their latency
    const int64_t g0 = (int64_t)blockIdx.x * (kBlock * U);
    const int gn = (int)(a.ng - g0 < kBlock * U ? a.ng - g0 : kBlock * U);    // groups of this chunk (0: a tensor without a body)
    const int64_t e0 = a.head + 8 * g0;
    const u4v *xv = reinterpret_cast<const u4v *>(x + e0);
    u4v v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (tid + u * kBlock < gn) v[u] = NT ? __builtin_nontemporal_load(xv + tid + u * kBlock) : xv[tid + u * kBlock];

    if (blockIdx.x == 0) {   // the scalars around the body: no table, the exact scale directly
        const int64_t tail0 = a.head + 8 * a.ng;
        int64_t e = -1;
        if (tid < a.head)
            e = tid;
        else if (tid >= 32 && tail0 + (tid - 32) < a.n)
            e = tail0 + (tid - 32);
        if (e >= 0) {
            const Chan c = make_chan(maxval[PC ? e / a.inner : 0], f);
            store1<T, YF32>(y, e, quant_direct(T::widen1(x[e]), c, f.M));
        }
    }
    if (gn <= 0) return;

    int64_t row_lo = 0;
    int phase = 0, nrows = 1;
    if (PC) {
        row_lo = e0 / a.inner;
        phase = (int)(e0 - row_lo * a.inner);
        nrows = (int)(((int64_t)phase + 8 * gn - 1) / a.inner) + 1;
    }
    // four lanes per row share a table (lut_part): 256 threads build 64 rows at once
    for (int t = tid; t < nrows * 4; t += kBlock) {
        const int lr = t >> 2, sub = t & 3;
        const Chan c = make_chan(maxval[PC ? row_lo + lr : 0], f);
        if (sub == 0) chl[lr] = make_float4(c.maxv, c.minv, c.bias, c.pthr);
        lut_part(lut + lr * a.lut_stride, c, f, sub, 4);
    }
    __syncthreads();

#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int q = tid + u * kBlock;
        if (q >= gn) break;
        float e[8];
        T::widen2(v[u].x, e[0], e[1]);
        T::widen2(v[u].y, e[2], e[3]);
        T::widen2(v[u].z, e[4], e[5]);
        T::widen2(v[u].w, e[6], e[7]);
        int lr = 0, b = 8;
        if (PC) {
            const uint32_t o = (uint32_t)phase + 8u * (uint32_t)q;
            lr = a.inner >= CH ? (int)((int64_t)o >= a.inner) : div_small(o, a.magic);
            b = (int)(a.inner - ((int64_t)o - (int64_t)lr * a.inner));   // elements left in this row (>= 1)
        }
        const float2 *lt = lut + lr * a.lut_stride;
        if (PC) {
            // e[b..7] belong to the next row (rows hold >= 8 elements: exactly one more row): every element takes its own
            // row's constants and table -- five selects per element, no second evaluation of the group
            const int lrn = lr + 1 < nrows ? lr + 1 : lr;
            quant_group_2rows(e, b, lite_of(chl[lr]), lt, lite_of(chl[lrn]), lut + lrn * a.lut_stride, pmaxf, f.qthr);
        } else {
            quant_group<8>(e, lite_of(chl[lr]), lt, pmaxf, f.qthr);
        }
        if (YF32) {
            float *yo = reinterpret_cast<float *>(y) + e0 + 8 * (int64_t)q;
            st16u<NT>(yo, vf4{e[0], e[1], e[2], e[3]});
            st16u<NT>(yo + 4, vf4{e[4], e[5], e[6], e[7]});
        } else {
            u4v2 *yo = reinterpret_cast<u4v2 *>(reinterpret_cast<uint16_t *>(y) + e0 + 8 * (int64_t)q);
            const u4v2 w = {T::narrow2(e[0], e[1]), T::narrow2(e[2], e[3]), T::narrow2(e[4], e[5]), T::narrow2(e[6], e[7])};
            if (NT)
                __builtin_nontemporal_store(w, yo);
            else
                *yo = w;
        }
    }
}

// thread = row, no table: per-channel rows the chunk kernel does not take
template <class T, bool YF32>
__global__ void __launch_bounds__(kBlock)
k_h16_quant_rows(const uint16_t *x, void *y, int64_t C, int64_t inner,
                 const float *__restrict__ maxval, QFmt f)
{
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= C) return;
    const Chan c = make_chan(maxval[row], f);
    for (int64_t j = 0; j < inner; ++j) {
        const int64_t e = row * inner + j;
        store1<T, YF32>(y, e, quant_direct(T::widen1(x[e]), c, f.M));
    }
}

// ---------------------------------------------------------------------------------------------
// min / max
// ---------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void mm_acc8(MinMax &m, const u4v w)
{
    float a, b;
    T::widen2(w.x, a, b);
    mm_acc(m, a);
    mm_acc(m, b);
    T::widen2(w.y, a, b);
    mm_acc(m, a);
    mm_acc(m, b);
    T::widen2(w.z, a, b);
    mm_acc(m, a);
    mm_acc(m, b);
    T::widen2(w.w, a, b);
    mm_acc(m, a);
    mm_acc(m, b);
}

template <class T>
__global__ void __launch_bounds__(kBlock)
k_h16_minmax_rows(const uint16_t *__restrict__ x, int64_t C, int inner, int gs, float *cur_min, float *cur_max,
                  float *maxval_out, FoldArgs fa)
{
    const int G = 1 << gs, tid = threadIdx.x, sub = tid & (G - 1);
    const int64_t row = (int64_t)blockIdx.x * (kBlock >> gs) + (tid >> gs);
    MinMax m;
    mm_init(m);
    if (row < C) {
        // 16 bytes (8 elements) per lane and access at whatever 2-byte phase the row starts; the G lanes of a row, and the
        // rows of a block, cover contiguous memory.  The last inner % 8 elements are scalars.
        const uint16_t *xr = x + row * inner;
        const int nv = inner >> 3;
        for (int k = sub; k < nv; k += G) {
            const u4v2 w = *reinterpret_cast<const u4v2 *>(xr + 8 * k);
            mm_acc8<T>(m, u4v{w.x, w.y, w.z, w.w});
        }
        for (int j = (nv << 3) + sub; j < inner; j += G) mm_acc(m, T::widen1(xr[j]));
    }
    for (int off = G >> 1; off >= 1; off >>= 1) {
        m.mn = fminf(m.mn, __shfl_xor(m.mn, off, 64));
        m.mx = fmaxf(m.mx, __shfl_xor(m.mx, off, 64));
        m.nan |= __shfl_xor(m.nan, off, 64);
    }
    if (row < C && sub == 0) {
        if (m.nan) m.mn = m.mx = __builtin_nanf("");
        fold_store(m.mn, m.mx, row, cur_min, cur_max, maxval_out, fa);
    }
}

template <class T, bool NT>
__global__ void __launch_bounds__(kBlock)
k_h16_minmax_part(const uint16_t *__restrict__ x, int64_t inner, int nsplit, unsigned long long *slots, unsigned tag,
                  float *cur_min, float *cur_max, float *maxval_out, FoldArgs fa)
{
    if ((int)blockIdx.x == nsplit) {   // only launched when nsplit > 1
        block_minmax_collect(slots + (int64_t)blockIdx.y * nsplit * 2, nsplit, tag, blockIdx.y, cur_min, cur_max,
                             maxval_out, fa);
        return;
    }
    const int row = blockIdx.y, split = blockIdx.x, tid = threadIdx.x;
    const uint16_t *xr = x + (int64_t)row * inner;
    MinMax m;
    mm_init(m);
    int64_t head = ((16 - ((uintptr_t)xr & 15)) & 15) >> 1;
    if (head > inner) head = inner;
    const int64_t nvec = (inner - head) >> 3;
    const int64_t tail0 = head + (nvec << 3);
    if (split == 0) {
        if (tid < head) mm_acc(m, T::widen1(xr[tid]));
        if (tail0 + tid < inner) mm_acc(m, T::widen1(xr[tail0 + tid]));
    }
    const u4v *xv = reinterpret_cast<const u4v *>(xr + head);
    constexpr int U = 8;
    const int64_t step = (int64_t)nsplit * (kBlock * U);
    for (int64_t base = (int64_t)split * (kBlock * U); base < nvec; base += step) {
        if (base + kBlock * U <= nvec) {
            u4v v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                v[u] = NT ? __builtin_nontemporal_load(xv + base + u * kBlock + tid) : xv[base + u * kBlock + tid];
#pragma unroll
            for (int u = 0; u < U; ++u) mm_acc8<T>(m, v[u]);
        } else {
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + u * kBlock + tid;
                if (i < nvec) mm_acc8<T>(m, xv[i]);
            }
        }
    }
    block_minmax_publish(m, slots + (int64_t)row * nsplit * 2, split, nsplit, tag, row, cur_min, cur_max, maxval_out, fa);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
constexpr int kRowsMmMaxInner = 2048;   // k_h16_minmax_rows up to here

// What a K1 call launches: every decision of the launcher, taken once from the shape, the format and x's 16-byte phase.
// quant_launch consumes it; fp8q_h16_route reports it.
struct QuantPlan {
    int kernel;       // FP8Q_H16_K_QUANT / FP8Q_H16_K_QUANT_ROWS
    int u;            // k_h16_quant: 16-byte groups in flight per lane (1, 4)
    bool nt;          // the nontemporal instance (U = 4 only)
    H16Args a;
    size_t shmem;
    int64_t grid_x;
};

QuantPlan quant_plan(uintptr_t x, int64_t C, int64_t inner, bool pc, const QFmt &f)
{
    QuantPlan p = {};
    H16Args &a = p.a;
    a.n = C * inner;
    a.head = ((16 - (x & 15)) & 15) >> 1;
    if (a.head > a.n) a.head = a.n;
    a.ng = (a.n - a.head) >> 3;
    a.inner = pc ? inner : a.n;
    a.lut_stride = f.pmax + 1;
    const size_t per_row = sizeof(float4) + (size_t)a.lut_stride * sizeof(float2);
    // U = 4 (16 KiB of half per block) for tensors that fill the chip with such blocks, else 1; per channel the tables of
    // the rows a chunk overlaps must fit the LDS budget
    int u = a.ng >= (int64_t)kBlock * 4 * 1024 ? 4 : 1;
    auto rows_of = [&](int uu) { return pc ? (int64_t)(kBlock * 8 * uu - 1) / inner + 2 : (int64_t)1; };
    if (pc) {
        if (u == 4 && rows_of(4) * per_row > kH16LdsBudget) u = 1;
        if (inner < 8 || rows_of(1) * per_row > kH16LdsBudget) {
            p.kernel = FP8Q_H16_K_QUANT_ROWS;
            p.grid_x = cdiv(C, kBlock);
            return p;
        }
    }
    p.kernel = FP8Q_H16_K_QUANT;
    p.u = u;
    a.nc_max = (int)rows_of(u);
    a.magic = (pc && inner < kBlock * 8 * u) ? magic_of((int)inner) : 0u;
    p.shmem = (size_t)a.nc_max * per_row;
    p.grid_x = a.ng > 0 ? cdiv(a.ng, (int64_t)kBlock * u) : 1;
    p.nt = u == 4 && a.n * 2 >= kNtBytes;   // (U = 1 has no nontemporal instance: 2^20 groups come long before 64 MiB)
    return p;
}

template <class T, bool YF32, bool PC>
void quant_launch_u(const QuantPlan &p, hipStream_t st, const uint16_t *x, void *y, const float *maxval, const QFmt &f)
{
    const dim3 g((unsigned)p.grid_x);
    if (p.u == 1)
        hipLaunchKernelGGL((k_h16_quant<T, YF32, PC, 1, false>), g, dim3(kBlock), p.shmem, st, x, y, maxval, f, p.a);
    else if (p.nt)
        hipLaunchKernelGGL((k_h16_quant<T, YF32, PC, 4, true>), g, dim3(kBlock), p.shmem, st, x, y, maxval, f, p.a);
    else
        hipLaunchKernelGGL((k_h16_quant<T, YF32, PC, 4, false>), g, dim3(kBlock), p.shmem, st, x, y, maxval, f, p.a);
}

template <class T, bool YF32>
int quant_launch(const uint16_t *x, void *y, int64_t C, int64_t inner, const float *maxval, bool pc, const QFmt &f,
                 hipStream_t st)
{
    const QuantPlan p = quant_plan((uintptr_t)x, C, inner, pc, f);
    if (p.kernel == FP8Q_H16_K_QUANT_ROWS)
        hipLaunchKernelGGL((k_h16_quant_rows<T, YF32>), dim3((unsigned)p.grid_x), dim3(kBlock), 0, st, x, y, C, inner, maxval, f);
    else if (pc)
        quant_launch_u<T, YF32, true>(p, st, x, y, maxval, f);
    else
        quant_launch_u<T, YF32, false>(p, st, x, y, maxval, f);
    return launch_rc();
}

int quant_dispatch(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *maxval, bool pc,
                   const QFmt &f, hipStream_t st)
{
    const uint16_t *xs = (const uint16_t *)x;
    const bool yf32 = y_type == FP8Q_DT_F32;
    if (x_type == FP8Q_DT_F16)
        return yf32 ? quant_launch<F16, true>(xs, y, C, inner, maxval, pc, f, st) : quant_launch<F16, false>(xs, y, C, inner, maxval, pc, f, st);
    return yf32 ? quant_launch<BF16, true>(xs, y, C, inner, maxval, pc, f, st) : quant_launch<BF16, false>(xs, y, C, inner, maxval, pc, f, st);
}

// shared argument checks of the two quantizing entry points (everything is reported before any launch)
int quant_check(const void *x, const void *y, int x_type, int y_type, int64_t C, int64_t inner, bool pc, float mbits,
                int n_bits, int sign_bits, QFmt *f)
{
    if (int rc = check_types(x_type, y_type)) return rc;
    if (!x || !y || C <= 0 || inner <= 0) return FP8Q_EINVAL;
    if (int rc = make_fmt(mbits, n_bits, sign_bits, f)) return rc;
    if (((uintptr_t)x & 1) || ((uintptr_t)y & (y_type == FP8Q_DT_F32 ? 3 : 1))) return FP8Q_EINVAL;
    // per channel the chunk-local offsets are 32-bit (rows up to 2^30 elements); chunk counts fit gridDim.x
    if ((pc && inner > (1 << 30)) || C > INT64_MAX / inner || cdiv(C * inner, 8 * kBlock) > (int64_t)INT32_MAX) return FP8Q_EINVAL;
    return FP8Q_OK;
}

// how many streaming blocks a row may have so that the workspace of fp8q_minmax_workspace_bytes(C, inner) holds their granules
int minmax_h16_nsplit(int64_t C, int64_t inner)
{
    const size_t bytes = fp8q_minmax_workspace_bytes(C, inner);
    const int64_t avail = bytes > kMinmaxWsHeader ? (int64_t)((bytes - kMinmaxWsHeader) / ((size_t)C * 16)) : 1;
    const int64_t want = balanced_blocks(cdiv(cdiv(inner, 8), kBlock * 8), kTargetBlocks / C);
    const int64_t ns = want < avail ? want : avail;
    return (int)(ns < 1 ? 1 : ns);
}

// What a min/max call launches, from the shape alone (need_ws: the entry with a workspace, whose long rows may be split).
// minmax_launch consumes it; fp8q_h16_route reports it.
struct MinmaxPlan {
    int kernel;        // FP8Q_H16_K_MINMAX_ROWS / FP8Q_H16_K_MINMAX_PART
    int gs;            // k_h16_minmax_rows: 2^gs lanes per row
    int ns;            // k_h16_minmax_part: streaming blocks per row
    bool nt;
    unsigned gx;
    int64_t gy;        // of the first launch
    int launches;      // slabs of 65535 rows
};

constexpr int64_t kMmSlabRows = 65535;   // gridDim.y

MinmaxPlan minmax_plan(int64_t C, int64_t inner, bool need_ws)
{
    MinmaxPlan p = {};
    p.launches = 1;
    if (C > 1 && inner <= kRowsMmMaxInner) {
        p.kernel = FP8Q_H16_K_MINMAX_ROWS;
        while (p.gs < 6 && (32 << p.gs) < inner) ++p.gs;   // up to four 16-byte accesses per lane
        p.gx = (unsigned)cdiv(C, kBlock >> p.gs);
        p.gy = 1;
        return p;
    }
    p.kernel = FP8Q_H16_K_MINMAX_PART;
    p.ns = need_ws ? minmax_h16_nsplit(C, inner) : 1;
    p.gx = p.ns > 1 ? (unsigned)p.ns + 1u : 1u;   // + the row's reducer block
    p.gy = C < kMmSlabRows ? C : kMmSlabRows;
    p.nt = C * inner * 2 >= kNtBytes;
    p.launches = (int)cdiv(C, kMmSlabRows);   // ns > 1 implies C <= kTargetBlocks / 2: a single slab
    return p;
}

template <class T>
int minmax_launch(const uint16_t *x, int64_t C, int64_t inner, float *cur_min, float *cur_max, float *maxval_out, FoldArgs fa,
                  void *ws, size_t ws_bytes, bool need_ws, hipStream_t st)
{
    const MinmaxPlan p = minmax_plan(C, inner, need_ws);
    if (p.kernel == FP8Q_H16_K_MINMAX_ROWS) {
        hipLaunchKernelGGL(k_h16_minmax_rows<T>, dim3(p.gx), dim3(kBlock), 0, st, x, C, (int)inner, p.gs, cur_min, cur_max,
                           maxval_out, fa);
        return launch_rc();
    }
    unsigned long long *slots = nullptr;
    if (need_ws) {
        if (!ws || ws_bytes < fp8q_minmax_workspace_bytes(C, inner) || ((uintptr_t)ws & 7)) return FP8Q_EWORKSPACE;
        fa.status = (unsigned *)ws;
        fold_debug_env(fa);
        slots = (unsigned long long *)((char *)ws + kMinmaxWsHeader);
    }
    const unsigned tag = next_minmax_tag();
    for (int64_t c0 = 0; c0 < C; c0 += kMmSlabRows) {
        const int64_t cn = (C - c0) < kMmSlabRows ? (C - c0) : kMmSlabRows;
        const dim3 g(p.gx, (unsigned)cn);
        if (p.nt)
            hipLaunchKernelGGL((k_h16_minmax_part<T, true>), g, dim3(kBlock), 0, st, x + c0 * inner, inner, p.ns, slots, tag,
                               cur_min ? cur_min + c0 : nullptr, cur_max ? cur_max + c0 : nullptr,
                               maxval_out ? maxval_out + c0 : nullptr, fa);
        else
            hipLaunchKernelGGL((k_h16_minmax_part<T, false>), g, dim3(kBlock), 0, st, x + c0 * inner, inner, p.ns, slots, tag,
                               cur_min ? cur_min + c0 : nullptr, cur_max ? cur_max + c0 : nullptr,
                               maxval_out ? maxval_out + c0 : nullptr, fa);
        if (int rc = launch_rc()) return rc;
    }
    return FP8Q_OK;
}

int minmax_dispatch(const void *x, int x_type, int64_t C, int64_t inner, float *cur_min, float *cur_max, float *maxval_out,
                    const FoldArgs &fa, void *ws, size_t ws_bytes, bool need_ws, hipStream_t st)
{
    const uint16_t *xs = (const uint16_t *)x;
    if (x_type == FP8Q_DT_F16) return minmax_launch<F16>(xs, C, inner, cur_min, cur_max, maxval_out, fa, ws, ws_bytes, need_ws, st);
    return minmax_launch<BF16>(xs, C, inner, cur_min, cur_max, maxval_out, fa, ws, ws_bytes, need_ws, st);
}

// the shape checks of fp8q_minmax_h16 and of the fused entry behind quant_check (shared with fp8q_h16_route)
int minmax_check(const void *x, int64_t C, int64_t inner)
{
    if (!x || C <= 0 || inner <= 0 || ((uintptr_t)x & 1)) return FP8Q_EINVAL;
    if (C > INT64_MAX / inner) return FP8Q_EINVAL;
    return FP8Q_OK;
}

int fused_check(int64_t inner) { return inner > fp8q_fused_max_inner() ? FP8Q_ETOOLONG : FP8Q_OK; }

void report(const QuantPlan &p, fp8q_h16_launch_info &r)
{
    r.kernel = p.kernel;
    r.launches = 1;
    r.grid_x = p.grid_x;
    r.grid_y = 1;
    if (p.kernel != FP8Q_H16_K_QUANT) return;
    r.u = p.u;
    r.nontemporal = p.nt;
    r.head = p.a.head;
    r.groups = p.a.ng;
    r.tail = p.a.n - p.a.head - 8 * p.a.ng;
    r.rows_per_chunk = p.a.nc_max;
    r.lds_bytes = (int64_t)p.shmem;
}

void report(const MinmaxPlan &p, fp8q_h16_launch_info &r)
{
    r.kernel = p.kernel;
    r.launches = p.launches;
    r.grid_x = p.gx;
    r.grid_y = p.gy;
    if (p.kernel == FP8Q_H16_K_MINMAX_ROWS) {
        r.lanes = 1 << p.gs;
    } else {
        r.nsplit = p.ns;
        r.nontemporal = p.nt;
    }
}

}  // namespace

extern "C" {

// Which kernels the three entries below launch: their argument checks and their launchers' plans (quant_plan, minmax_plan) on
// made-up addresses that have the caller's 16-byte phase and are never dereferenced.  Host arithmetic only.
int fp8q_h16_route(int op, int64_t C, int64_t inner, int per_channel, float mbits, int n_bits, int sign_bits, int x_mod16,
                   int y_type, fp8q_h16_route_info *info)
{
    if (!info || op < FP8Q_ROWS_QUANTIZE || op > FP8Q_ROWS_MINMAX_QUANTIZE || x_mod16 < 0 || x_mod16 > 15) return FP8Q_EINVAL;
    if (y_type != FP8Q_DT_F32 && !half_type(y_type)) return FP8Q_EINVAL;
    if (op == FP8Q_ROWS_MINMAX_QUANTIZE && !per_channel) return FP8Q_EINVAL;
    const void *x = reinterpret_cast<const void *>(((uintptr_t)1 << 44) + (uintptr_t)x_mod16);
    void *y = reinterpret_cast<void *>((uintptr_t)1 << 45);
    const int x_type = half_type(y_type) ? y_type : FP8Q_DT_F16;   // (the route is the same for both half types)
    fp8q_h16_route_info r = {};
    QFmt f;
    if (op == FP8Q_ROWS_MINMAX) {
        if (!per_channel && C > 0 && inner > 0) {   // the wrapper's view of a per-tensor estimator: one row
            if (C > INT64_MAX / inner) return FP8Q_EINVAL;
            inner *= C;
            C = 1;
        }
        if (int rc = minmax_check(x, C, inner)) return rc;
        report(minmax_plan(C, inner, true), r.launch[r.n_launches++]);
    } else {
        if (int rc = quant_check(x, y, x_type, y_type, C, inner, per_channel != 0, mbits, n_bits, sign_bits, &f)) return rc;
        if (op == FP8Q_ROWS_MINMAX_QUANTIZE) {
            if (int rc = fused_check(inner)) return rc;
            report(minmax_plan(C, inner, false), r.launch[r.n_launches++]);
        }
        report(quant_plan((uintptr_t)x, C, inner, per_channel != 0, f), r.launch[r.n_launches++]);
    }
    *info = r;
    return FP8Q_OK;
}

int fp8q_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *maxval,
                      int64_t n_maxval, float mbits, int n_bits, int sign_bits, fp8q_stream_t stream)
{
    QFmt f;
    if (int rc = quant_check(x, y, x_type, y_type, C, inner, n_maxval != 1, mbits, n_bits, sign_bits, &f)) return rc;
    if (!maxval || (n_maxval != 1 && n_maxval != C)) return FP8Q_EINVAL;
    return quant_dispatch(x, y, x_type, y_type, C, inner, maxval, n_maxval != 1, f, (hipStream_t)stream);
}

int fp8q_minmax_h16(const void *x, int x_type, int64_t C, int64_t inner, float *cur_min, float *cur_max, float *maxval_out,
                    int fold_mode, double momentum, int first, void *ws, size_t ws_bytes, fp8q_stream_t stream)
{
    if (!half_type(x_type)) return FP8Q_EINVAL;
    if (!cur_min || !cur_max || fold_mode < 0 || fold_mode > 2) return FP8Q_EINVAL;
    if (int rc = minmax_check(x, C, inner)) return rc;
    FoldArgs fa;
    fa.mode = fold_mode;
    fa.first = first != 0;
    fa.om = (float)(1.0 - momentum);
    fa.mo = (float)momentum;
    return minmax_dispatch(x, x_type, C, inner, cur_min, cur_max, maxval_out, fa, ws, ws_bytes, true, (hipStream_t)stream);
}

int fp8q_minmax_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, float *row_min,
                             float *row_max, float *maxval_out, float mbits, int n_bits, int sign_bits, fp8q_stream_t stream)
{
    QFmt f;
    if (int rc = quant_check(x, y, x_type, y_type, C, inner, true, mbits, n_bits, sign_bits, &f)) return rc;
    if (!maxval_out) return FP8Q_EINVAL;   // carries the ranges from the scan to K1
    if (int rc = fused_check(inner)) return rc;
    FoldArgs fa;
    fa.mode = FP8Q_FOLD_CURRENT;
    fa.first = 1;
    fa.om = fa.mo = 0.0f;
    hipStream_t st = (hipStream_t)stream;
    // rows up to fp8q_fused_max_inner(): one block (or 2^gs lanes) per row, no workspace
    if (int rc = minmax_dispatch(x, x_type, C, inner, row_min, row_max, maxval_out, fa, nullptr, 0, false, st)) return rc;
    return quant_dispatch(x, y, x_type, y_type, C, inner, maxval_out, true, f, st);
}

}  // extern "C"
