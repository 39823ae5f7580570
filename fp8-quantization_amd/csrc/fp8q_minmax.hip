// fp8q_minmax.hip -- K2/K3 of the quantize / min-max family (file map: fp8q_quant.hip): the single-launch min/max of long
// rows, its workspace, the packed / linspace variants, the sign fold.  Short rows: the launchers of fp8q_rows.h.
#include <vector>

#include "fp8q_rows.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K2/K3: min / max / NaN of x[row, split range], published as tagged granules; block nsplit of a row is the row's
// reducer (block_minmax_publish / block_minmax_collect, fp8q_common.h): one launch.
// ---------------------------------------------------------------------------------------------
template <bool NT>
__global__ void __launch_bounds__(kBlock)
k_minmax_partial(const float *__restrict__ x, int64_t inner, int nsplit, unsigned long long *slots, unsigned tag,
                 float *cur_min, float *cur_max, float *maxval_out, FoldArgs fa)
{
    if ((int)blockIdx.x == nsplit) {   // only launched when nsplit > 1
        block_minmax_collect(slots + (int64_t)blockIdx.y * nsplit * 2, nsplit, tag, blockIdx.y, cur_min, cur_max,
                             maxval_out, fa);
        return;
    }
    const int row = blockIdx.y, split = blockIdx.x, tid = threadIdx.x;
    const float *xr = x + (int64_t)row * inner;
    MinMax m;
    mm_init(m);
    int64_t head = ((16 - ((uintptr_t)xr & 15)) & 15) >> 2;
    if (head > inner) head = inner;
    const int64_t nvec = (inner - head) >> 2;
    const int64_t tail0 = head + (nvec << 2);
    if (split == 0) {
        if (tid < head) mm_acc(m, xr[tid]);
        if (tail0 + tid < inner) mm_acc(m, xr[tail0 + tid]);
    }
    const vf4 *xv = reinterpret_cast<const vf4 *>(xr + head);
    constexpr int U = 8;
    const int64_t step = (int64_t)nsplit * (kBlock * U);
    for (int64_t base = (int64_t)split * (kBlock * U); base < nvec; base += step) {
        if (base + kBlock * U <= nvec) {
            vf4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = ld16<NT>(xv + base + u * kBlock + tid);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                mm_acc(m, v[u].x);
                mm_acc(m, v[u].y);
                mm_acc(m, v[u].z);
                mm_acc(m, v[u].w);
            }
        } else {
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + u * kBlock + tid;
                if (i < nvec) {
                    const vf4 w = ld16<NT>(xv + i);
                    mm_acc(m, w.x);
                    mm_acc(m, w.y);
                    mm_acc(m, w.z);
                    mm_acc(m, w.w);
                }
            }
        }
    }
    block_minmax_publish(m, slots + (int64_t)row * nsplit * 2, split, nsplit, tag, row, cur_min, cur_max, maxval_out, fa);
}

// After the all-reduce(MAX) of the packed ranges of batch-sharded calibration (FoldArgs::packed, fold_store): back to
// {min, max} (+ K5: maxval = |max(|min|, max)|, fp8_quantizer.py:236) -- one launch instead of ~8 tiny tensor ops.
__global__ void __launch_bounds__(kBlock)
k_ranges_unpack(const float *__restrict__ packed, int64_t n, float *cur_min, float *cur_max, float *maxval_out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = reinterpret_cast<const float4 *>(packed)[i];
    const float nan = __builtin_nanf("");
    const float mn = p.z > 0.0f ? nan : -p.x, mx = p.w > 0.0f ? nan : p.y;
    if (cur_min) cur_min[i] = mn;
    if (cur_max) cur_max[i] = mx;
    if (maxval_out) maxval_out[i] = fabsf(tmax(fabsf(mn), mx));
}

}  // namespace

extern "C" {

// FPQuantizer.set_quant_range's sign decision (fp8_quantizer.py:216-225: `allow_unsigned and torch.all(x_min >= 0)` ->
// sign_bits = 0, never back) on the device: signed_flag[0] stays 1 only while some range minimum is not >= 0 (NaN: signed).
__global__ void __launch_bounds__(kBlock) k_sign_fold(const float *__restrict__ x_min, int64_t C, unsigned char *flag)
{
    __shared__ int s_any;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    int any = 0;
    for (int64_t i = threadIdx.x; i < C; i += kBlock) any |= !(x_min[i] >= 0.0f);
    if (any) s_any = 1;
    __syncthreads();
    if (threadIdx.x == 0 && !s_any) flag[0] = 0;
}

int fp8q_sign_fold_u8(const float *x_min, int64_t C, unsigned char *signed_flag, fp8q_stream_t stream)
{
    if (C < 0 || !signed_flag || (C > 0 && !x_min)) return FP8Q_EINVAL;
    hipLaunchKernelGGL(k_sign_fold, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, x_min, C, signed_flag);
    return launch_rc();
}

static int minmax_nsplit(int64_t C, int64_t inner)
{
    static const int cap_env = [] {   // FP8Q_K3_BLOCKS: streaming blocks of the two-stage min/max (tuning knob)
        const char *e = getenv("FP8Q_K3_BLOCKS");
        const int v = e ? atoi(e) : 0;
        return v >= 1 && v <= kTargetBlocks ? v : kTargetBlocks;   // <= 2048: split rows keep their reducers <= 1024 (progress argument, fp8q_common.h)
    }();
    return (int)balanced_blocks(cdiv(cdiv(inner, 4), kBlock * 8), cap_env / (C > 0 ? C : 1));
}

size_t fp8q_minmax_workspace_bytes(int64_t C, int64_t inner)
{
    if (C <= 0 || inner <= 0) return 16;
    if (inner <= fp8q_direct_max_inner() && C > 1) return 16;  // short-row path needs none
    const int ns = minmax_nsplit(C, inner);
    // the 16-byte header {timeout count, reserved} + two tagged granules per part
    return ns > 1 ? kMinmaxWsHeader + (size_t)C * (size_t)ns * 2 * sizeof(unsigned long long) : kMinmaxWsHeader;
}

// Synchronising check of a min/max workspace (fp8q_minmax_workspace_check; also run on entry by every min/max call
// under FP8Q_DEBUG_WS=1): the header's timeout count and the "all granules zero between calls" contract.
static int minmax_ws_check(void *ws, size_t ws_bytes, int clear, hipStream_t st)
{
    if (!ws || ws_bytes < kMinmaxWsHeader || ((uintptr_t)ws & 7)) return FP8Q_EWORKSPACE;
    if (hipError_t e = hipStreamSynchronize(st)) return (int)e;
    std::vector<unsigned long long> host(ws_bytes / 8);
    if (hipError_t e = hipMemcpy(host.data(), ws, host.size() * 8, hipMemcpyDeviceToHost)) return (int)e;
    const unsigned timeouts = (unsigned)host[0];
    bool dirty = false;
    for (size_t i = kMinmaxWsHeader / 8; i < host.size(); ++i) dirty |= host[i] != 0ull;
    if (clear && (timeouts || dirty)) {
        if (hipError_t e = hipMemsetAsync(ws, 0, ws_bytes, st)) return (int)e;
        if (hipError_t e = hipStreamSynchronize(st)) return (int)e;
    }
    if (timeouts) return FP8Q_ETIMEDOUT;
    return dirty ? FP8Q_EWORKSPACE : FP8Q_OK;
}

static bool minmax_debug_ws()
{
    static const bool on = env_int("FP8Q_DEBUG_WS", 0) != 0;
    return on;
}

struct LinArgs {
    float *grid = nullptr;
    int steps = 0;
    double lo = 0.0, hi = 0.0;
};

static int minmax_impl(const float *x, int64_t C, int64_t inner, float *cur_min, float *cur_max, float *maxval_out,
                       float *packed, int fold_mode, double momentum, int first, void *ws, size_t ws_bytes,
                       fp8q_stream_t stream, LinArgs lin = LinArgs(), fp8q_rows_route_info *rec = nullptr)
{
    if (!x || !cur_min || !cur_max || C <= 0 || inner <= 0 || fold_mode < 0 || fold_mode > 2)
        return FP8Q_EINVAL;
    if (packed && ((uintptr_t)packed & 15)) return FP8Q_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    FoldArgs fa;
    fa.mode = fold_mode;
    fa.first = first != 0;
    fa.om = (float)(1.0 - momentum);
    fa.mo = (float)momentum;
    fa.packed = packed;
    fa.lin_grid = lin.grid;
    fa.lin_steps = lin.steps;
    fa.lin_C = C;
    fa.lin_lo = lin.lo;
    fa.lin_hi = lin.hi;
    // (the row-kernel launchers below cut C into slabs themselves and pass slab-local rows to fold_store together with
    // slab-offset range pointers, while the grid / table base stays that of row 0: tables per row need C <= 65535 there)
    if (lin.grid && C > 65535) return FP8Q_ETOOMANY;
    if (C > 1) {   // per-channel rows of 128..8192 elements: one launch, the row in registers
        QFmt f = {};
        const int rc = fp8q_launch_rows_reg(false, x, nullptr, C, inner, cur_min, cur_max, maxval_out, f, fa, st, rec);
        if (rc != kNotFlat) return rc;
    }
    if (C > 1) {   // short rows: aligned chunks through LDS
        const int rc = fp8q_launch_rows_staged_mm(x, C, inner, cur_min, cur_max, maxval_out, fa, st, rec);
        if (rc != kNotFlat) return rc;
    }
    if (inner <= fp8q_direct_max_inner() && C > 1 && ((uintptr_t)x & 3) == 0) {
        QFmt f = {};
        return fp8q_launch_rows_direct(kModeMinMax, x, nullptr, C, inner, nullptr, cur_min, cur_max, maxval_out,
                                  f, fa, st, rec);
    }
    // (a route query brings no workspace and takes no tag: everything else below is the launch's own arithmetic)
    if (!rec && (ws_bytes < fp8q_minmax_workspace_bytes(C, inner) || !ws || ((uintptr_t)ws & 7))) return FP8Q_EWORKSPACE;
    if (!rec && minmax_debug_ws())
        if (int rc = minmax_ws_check(ws, fp8q_minmax_workspace_bytes(C, inner), 0, st)) return rc;
    const int ns = minmax_nsplit(C, inner);
    const unsigned tag = rec ? 0u : next_minmax_tag();
    const unsigned gx = ns > 1 ? (unsigned)ns + 1u : 1u;   // + the row's reducer block
    fa.status = (unsigned *)ws;
    fold_debug_env(fa);
    unsigned long long *slots = (unsigned long long *)((char *)ws + kMinmaxWsHeader);
    for (int64_t c0 = 0; c0 < C; c0 += 65535) {   // ns > 1 implies C <= kTargetBlocks / 2: a single slab
        const int64_t cn = (C - c0) < 65535 ? (C - c0) : 65535;
        fa.packed = packed ? packed + 4 * c0 : nullptr;
        const bool nt = C * inner * 4 >= kNtBytes;
        const auto fill = [&](fp8q_rows_route_info &r) {
            r.kernel = FP8Q_ROWS_K_MINMAX_PARTIAL;
            r.nontemporal = nt;
            r.nsplit = ns;
            r.grid_x = gx;
            r.grid_y = cn;
        };
        const int rc = rows_emit(rec, fill, [&] {
            dispatch<true, false>(nt, [&](auto NT) {
                hipLaunchKernelGGL(k_minmax_partial<NT()>, dim3(gx, (unsigned)cn), dim3(kBlock), 0, st, x + c0 * inner, inner,
                                   ns, slots, tag, cur_min + c0, cur_max + c0, maxval_out ? maxval_out + c0 : nullptr, fa);
            });
        });
        if (rc) return rc;
    }
    return FP8Q_OK;
}

// fp8q_minmax_f32's route for fp8q_rows_route: minmax_impl with a record instead of a stream (overwrite fold, no workspace)
int fp8q_minmax_plan(const float *x, int64_t C, int64_t inner, fp8q_rows_route_info *rec)
{
    float *rng = reinterpret_cast<float *>((uintptr_t)1 << 46);
    return minmax_impl(x, C, inner, rng, rng, rng, nullptr, FP8Q_FOLD_CURRENT, 0.0, 1, nullptr, 0, nullptr, LinArgs(), rec);
}

int fp8q_minmax_f32(const float *x, int64_t C, int64_t inner, float *cur_min, float *cur_max,
                    float *maxval_out, int fold_mode, double momentum, int first, void *ws,
                    size_t ws_bytes, fp8q_stream_t stream)
{
    return minmax_impl(x, C, inner, cur_min, cur_max, maxval_out, nullptr, fold_mode, momentum, first, ws, ws_bytes, stream);
}

int fp8q_minmax_packed_f32(const float *x, int64_t C, int64_t inner, float *cur_min, float *cur_max,
                           float *maxval_out, float *packed, int fold_mode, double momentum, int first, void *ws,
                           size_t ws_bytes, fp8q_stream_t stream)
{
    if (!packed) return FP8Q_EINVAL;
    return minmax_impl(x, C, inner, cur_min, cur_max, maxval_out, packed, fold_mode, momentum, first, ws, ws_bytes, stream);
}

int fp8q_minmax_linspace_f32(const float *x, int64_t C, int64_t inner, float *cur_min, float *cur_max, float *maxval_out,
                             float *grid, int n_cand, double lo_frac, double hi_frac, void *ws, size_t ws_bytes,
                             fp8q_stream_t stream)
{
    if (!grid || !maxval_out || n_cand < 2 || n_cand > (1 << 20)) return FP8Q_EINVAL;
    LinArgs lin;
    lin.grid = grid;
    lin.steps = n_cand;
    lin.lo = lo_frac;
    lin.hi = hi_frac;
    return minmax_impl(x, C, inner, cur_min, cur_max, maxval_out, nullptr, FP8Q_FOLD_CURRENT, 0.0, 1, ws, ws_bytes, stream, lin);
}

int fp8q_minmax_workspace_check(void *ws, size_t ws_bytes, int clear, fp8q_stream_t stream)
{
    try {
        return minmax_ws_check(ws, ws_bytes, clear, (hipStream_t)stream);
    } catch (...) {
        return (int)hipErrorOutOfMemory;
    }
}

int fp8q_ranges_unpack_f32(const float *packed, int64_t n, float *cur_min, float *cur_max, float *maxval_out,
                           fp8q_stream_t stream)
{
    if (n < 0 || (n > 0 && (!packed || ((uintptr_t)packed & 15)))) return FP8Q_EINVAL;
    if (n == 0) return FP8Q_OK;
    hipLaunchKernelGGL(k_ranges_unpack, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, packed, n,
                       cur_min, cur_max, maxval_out);
    return launch_rc();
}

}  // extern "C"
