// fp8q_multi.hip -- the multi-tensor plan of the quantize / min-max family (file map: fp8q_quant.hip): k_multi_flat (K1 or
// storage codes of many tensors in one launch), its per-row range twin k_multi_rowmax, the fp8q_multi_* entry points.
#include <vector>

#include "fp8q_rows.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Multi-tensor K1: every weight tensor of a model in ONE launch (21 launches of ~7 us each for
// ResNet-18's 11.7 M weights are launch-bound; the data is 47 MB).  One block = one aligned 4096-element
// chunk of one tensor, processed exactly like a k_rows_flat<0> tile with a single chunk; the tensor of a
// block comes from a <= 32-entry table passed by value in the kernel arguments (no device-side table,
// no workspace, no host-to-device copy).
// ---------------------------------------------------------------------------------------------
constexpr int kMultiMax = 32;

struct MultiDesc {
    const float *x;
    float *y;
    const float *maxval;
    int64_t nvec;        // 16-byte groups
    int inner;           // row length; per-tensor entries: the whole tensor is one row (single_row)
    int rpc;
    int tail;
    int single_row;
    uint32_t magic;
    uint32_t chunk0;     // first global chunk id of this tensor
    int n_bits;          // (storage codes: the sign bit's position)
    QFmt f;
};

struct MultiArgs {
    int n;
    int rpc_max;         // most table rows any chunk of any tensor needs
    uint32_t total_chunks;
    MultiDesc d[kMultiMax];
};

// One launch, every block resident at once (<= 1024 blocks: 4 per CU), chunks handed out grid-stride (neighbouring
// blocks on neighbouring chunks, a block's few chunks software-ordered: loads first, tables while they fly).  Round 2's
// version -- one chunk per block, 2850 blocks for ResNet-18 = 2.8 rounds -- spent most of its 24 us in per-block serial
// latency: a single thread's 64-bit software division, one thread per row building a whole table, a head-patch phase
// with dependent global loads, and only then the chunk's own loads.  Here: the chunk's loads are issued before anything
// else; the geometry is computed by every thread (double-precision quotient + fix-up: no LDS hand-off); a row's table
// is built by up to 32 lanes; the <= 3 elements of a 16-byte group that belong to the NEXT row are quantized in place
// with that row's table (a rare divergent branch) instead of a patch phase; the 3 KiB of log2 / exp2 tables are staged
// once per block, not once per chunk.
// Round 4 ablations on ResNet-18's 21 tensors (tools/ab.py multi, 93 MB of traffic; the plain copy of the same bytes:
// 14.2 us): this kernel 20.4 us; with the arithmetic removed (loads, tables, stores only) 16.2; with the tables of a
// block's first chunk reused for its other chunks 19.6 -- i.e. the per-chunk table phase costs ~1 us and the
// quantizer arithmetic ~4.5 us, which adds to the memory time instead of hiding under it: all ~1000 resident blocks
// start together and stay in phase (everybody loads, then everybody computes; 11.7 M elements x ~22 issue slots are
// ~6.5 us of a busy VALU), and at 3 chunks per block the kernel ends before the phases drift apart.  Requesting a
// block's next chunk right before the current chunk's arithmetic (16 more VGPRs: 100) did not change that (20.4 vs
// 20.1 us), nor did 950 / 1280 / 1425 / 2850 blocks (21.8 / 20.4 / 19.7 / 21.5 us).  One table phase for all of a
// block's chunks would remove at most the ~1 us the tables cost.  A fully software-pipelined variant was then written
// and measured (k_multi_flat_pipe, removed again): arithmetic into registers first, the next chunk's data AND the
// maxvals of its table rows requested before that arithmetic (unpredicated, fenced: the scheduler otherwise sinks the
// requests below the stores), descriptor index made provably uniform (readfirstlane) and the ballot key hoisted so
// that no vector load from the kernel-argument segment is left in the loop, one explicit s_waitcnt vmcnt(0) in front
// of the stores -- i.e. NO wait in the loop ever covers a store (gfx950's single in-order vmcnt would otherwise drain a
// chunk's stores before the next table phase; checked in the ISA) -- bit-exact, 117 VGPRs: 19.7 us by rocprofv3 against
// 19.9.  Counters of the plain kernel (rocprofv3 --pmc, per launch): 4.76 M VALU wave-instructions (418 per wave and
// chunk) = ~39 % of the VALU issue slots of a 19.9 us launch, 2.6 M SALU, LDS bank conflicts 1 % of LDS instructions,
// waves waiting 61 % of their cycles.  Neither memory latency, store drains, the table phase nor occupancy (1...3
// chunks per block measured equal) is THE limit; the launch is short enough (3 chunks per block) that its fixed phases
// (launch ramp, table staging, first load round trip, last compute + store drain) make up the gap to the copy.
// Round 5, the last structural attempt (profiles/r05_multi_stagger_ab.txt): blocks started out of phase -- block b waits
// (b % 4) x s x 0.9 us before its first load, so that a quarter of the chip computes while another quarter loads -- measured
// 19.96 / 21.7 / 23.6 / 25.8 / 28.3 us for s = 0 / 1 / 2 / 3 / 4 (rocprofv3, 170 launches each): every step of stagger is
// simply added to the launch, nothing overlaps better.  The phases are not what separates this launch from the copy; with 3
// chunks per block its fixed parts are (launch ramp, table staging, first round trip, last compute + store drain).  Closed.
// The launch replaces 21 launches (130 us from Python).
// MODE 0: K1 (fp32 -> fp32).  MODE 3 / 4 (round 5): the storage codes of N3 for many tensors at once -- encode (fp32 -> 1 byte,
// x = values, y = codes) / decode (1 byte -> fp32, x = codes, y = values): what the bucketed all-gather of channel-sharded
// weights packs into / unpacks from its send buffer in one launch each (fp8q_multi_minmax_encode_u8, fp8q_multi_decode_u8).
// Same chunks, tables and row bookkeeping; a group is 4 elements = one 16-byte load and one 4-byte store or vice versa.
template <int MODE>
__global__ void __launch_bounds__(kBlock, 4)
k_multi_flat(MultiArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double ftab[kFastTabSize];
    const int tid = threadIdx.x;
    float4 *chl = reinterpret_cast<float4 *>(smem);
    float2 *lut = reinterpret_cast<float2 *>(chl + a.rpc_max);
    for (int i = tid; i < kFastTabSize; i += kBlock) ftab[i] = kFastTab[i];
    constexpr int U = 4;
    // which tensor chunk g belongs to: lane l looks at descriptor l's first chunk, one ballot -- a scan over the
    // descriptors is up to 31 DEPENDENT scalar loads from the kernel-argument segment (~2 us for a model's last tensors)
    auto tensor_of = [&](uint32_t g) -> int {
        const int l = tid & 63;
        const uint32_t c0 = l < a.n ? a.d[l].chunk0 : 0xffffffffu;
        return __popcll(__ballot(c0 <= g)) - 1;   // chunk0 ascends from 0: uniform, >= 0
    };
    auto issue = [&](uint32_t g, int t, vf4 (&w)[U], uint32_t (&wc)[U]) {   // the chunk's groups of 4 elements: 4 per lane
        const MultiDesc &d = a.d[t];
        const int64_t elo = (int64_t)(g - d.chunk0) * kChunkElems;
        const int64_t rem = d.nvec * 4 - elo;
        const int ng = (rem < kChunkElems ? (int)rem : kChunkElems) >> 2;
        if (MODE == 4) {
            const uint32_t *xc = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(d.x) + elo);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (tid + u * kBlock < ng) wc[u] = xc[tid + u * kBlock];
        } else {
            const vf4 *xv = reinterpret_cast<const vf4 *>(d.x + elo);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (tid + u * kBlock < ng) w[u] = ld16<false>(xv + tid + u * kBlock);
        }
    };
    for (uint32_t g = blockIdx.x; g < a.total_chunks; g += gridDim.x) {
        const int t = tensor_of(g);
        vf4 v[U];
        uint32_t vc[U];
        issue(g, t, v, vc);   // in flight during the table phase (requesting the block's NEXT chunk here as well measured slower:
                          // 21.1 vs 19.1 us for ResNet-18's 21 tensors)
        const MultiDesc &d = a.d[t];
        const QFmt f = d.f;
        const int inner = d.inner, lut_stride = f.pmax + 1;
        const float pmaxf = (float)f.pmax;
        const int64_t elo = (int64_t)(g - d.chunk0) * kChunkElems;
        const float *x = d.x + elo;                                                       // (MODE 4: codes, see xb)
        float *y = d.y + elo;                                                             // (MODE 3: codes, see yb)
        const uint8_t *xb = reinterpret_cast<const uint8_t *>(d.x) + elo;
        uint8_t *yb = reinterpret_cast<uint8_t *>(d.y) + elo;
        const int Mi = (int)f.M, sign_shift = f.sign_bits == 1 ? d.n_bits - 1 : -1;
        const int64_t rem = d.nvec * 4 - elo;
        const int len = rem < kChunkElems ? (int)rem : kChunkElems;
        const int ng = len >> 2;
        const int tail = (rem <= kChunkElems) ? d.tail : 0;
        const int64_t row_lo = d.single_row ? 0 : div_rows(elo, inner);
        const int phase = d.single_row ? 0 : (int)(elo - row_lo * inner);
        const int nrows = d.single_row ? 1 : div_small((uint32_t)(phase + len + tail - 1), d.magic) + 1;
        __syncthreads();   // the previous chunk's tables are no longer read (first chunk: ftab is staged)
        {
            int gs = 0;   // log2(lanes per row): as many as hold all rows in one pass, at most 32
            while (gs < 5 && (nrows << (gs + 1)) <= kBlock) ++gs;
            const int L = 1 << gs, sub = tid & (L - 1);
            for (int r = tid >> gs; r < nrows; r += kBlock >> gs) {
                const Chan ch = make_chan_fast(d.maxval[d.single_row ? 0 : row_lo + r], f, ftab);
                if (sub == 0) chl[r] = make_float4(ch.maxv, ch.minv, ch.bias, ch.pthr);
                lut_part(lut + r * lut_stride, ch, f, sub, L);
            }
        }
        __syncthreads();
        if (tid < tail) {   // the tensor's last <= 3 elements
            const int e = len + tid;
            const int r = d.single_row ? 0 : div_small((uint32_t)(phase + e), d.magic);
            if (MODE == 3)
                yb[e] = (uint8_t)encode_one(x[e], lite_of(chl[r]), lut + r * lut_stride, pmaxf, f.qthr, Mi, sign_shift);
            else if (MODE == 4)
                y[e] = decode_one(xb[e], lut + r * lut_stride, Mi, sign_shift);
            else
                y[e] = quant_one(x[e], lite_of(chl[r]), lut + r * lut_stride, pmaxf, f.qthr);
        }
        vf4 *yv = reinterpret_cast<vf4 *>(y);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = tid + u * kBlock;
            if (q >= ng) break;
            const int o = phase + 4 * q;
            const int lrow = d.single_row ? 0 : div_small((uint32_t)o, d.magic);
            const int b = d.single_row ? 4 : inner - (o - lrow * inner);   // elements left in this row (>= 1)
            if (MODE == 4) {   // b..3 of the group are the next row's: its table
                const float2 *la = lut + lrow * lut_stride, *lb = la + lut_stride;
                const uint32_t w = vc[u];
                st16<false>(yv + q, vf4{decode_one(w & 255u, la, Mi, sign_shift), decode_one((w >> 8) & 255u, b > 1 ? la : lb, Mi, sign_shift),
                                        decode_one((w >> 16) & 255u, b > 2 ? la : lb, Mi, sign_shift),
                                        decode_one(w >> 24, b > 3 ? la : lb, Mi, sign_shift)});
                continue;
            }
            const float in[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            if (MODE == 3) {
                uint32_t wd = encode_group4(in, lite_of(chl[lrow]), lut + lrow * lut_stride, pmaxf, f.qthr, Mi, sign_shift);
                if (b < 4) {
                    const ChanLite cl = lite_of(chl[lrow + 1]);
                    const float2 *lt = lut + (lrow + 1) * lut_stride;
#pragma unroll
                    for (int k = 1; k < 4; ++k)
                        if (k >= b) wd = (wd & ~(255u << (8 * k))) | (encode_one(in[k], cl, lt, pmaxf, f.qthr, Mi, sign_shift) << (8 * k));
                }
                reinterpret_cast<uint32_t *>(yb)[q] = wd;
                continue;
            }
            float e[4] = {in[0], in[1], in[2], in[3]};
            quant_group<4>(e, lite_of(chl[lrow]), lut + lrow * lut_stride, pmaxf, f.qthr);
            if (b < 4) {   // e[b..3] belong to the next row (rows are >= 4 long: one boundary per group at most)
                const ChanLite cl = lite_of(chl[lrow + 1]);
                const float2 *lt = lut + (lrow + 1) * lut_stride;
#pragma unroll
                for (int k = 1; k < 4; ++k)
                    if (k >= b) e[k] = quant_one(in[k], cl, lt, pmaxf, f.qthr);
            }
            st16<false>(yv + q, vf4{e[0], e[1], e[2], e[3]});
        }
    }
}

// Per-channel ranges of MANY tensors in one launch: the estimate-state twin of k_multi_flat.  A model's weight tensors in
// estimate_ranges state (current_minmax, set_maxval: quantization_manager.py:114-122 per layer, i.e. one fused launch per
// layer = 21 launches of ~4 us for ResNet-18, or ~23 us each when driven from Python -- launch-bound either way) need
// every row's min / max before anything can be quantized.  Here one wave owns one row (rows of these tensors are
// 4 ... 16384 elements: 64 B ... 64 KiB), rows of all tensors are numbered consecutively, and the result
// maxval[c] = |max(|min_c|, max_c)| (fp8_quantizer.py:236) goes where k_multi_flat will read it: the two launches
// together are fp8q_multi_minmax_quantize_f32.  Dword loads (rows start at any 4-byte phase), coalesced per wave.
struct RowsDesc {
    const float *x;
    float *maxval;     // [C] output
    float *row_min;    // [C] output or nullptr
    float *row_max;
    int inner;
    uint32_t row0;     // first global row id of this tensor
};

struct RowsArgs {
    int n;
    uint32_t total_rows;
    RowsDesc d[kMultiMax];
};

__global__ void __launch_bounds__(kBlock)
k_multi_rowmax(RowsArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= a.total_rows) return;   // whole wave
    const uint32_t r0 = lane < a.n ? a.d[lane].row0 : 0xffffffffu;
    const int t = __popcll(__ballot(r0 <= row)) - 1;   // row0 ascends from 0
    const RowsDesc &d = a.d[t];
    const int64_t c = row - d.row0;
    const float *xr = d.x + c * d.inner;
    MinMax m;
    mm_init(m);
    int i = lane;
    for (; i + 192 < d.inner; i += 256) {   // four loads in flight per lane
        const float v0 = xr[i], v1 = xr[i + 64], v2 = xr[i + 128], v3 = xr[i + 192];
        mm_acc(m, v0);
        mm_acc(m, v1);
        mm_acc(m, v2);
        mm_acc(m, v3);
    }
    for (; i < d.inner; i += 64) mm_acc(m, xr[i]);
    mm_wave_reduce(m);
    if (lane == 0) {
        float mn = m.mn, mx = m.mx;
        if (m.nan) mn = mx = __builtin_nanf("");
        if (d.row_min) d.row_min[c] = mn;
        if (d.row_max) d.row_max[c] = mx;
        d.maxval[c] = fabsf(tmax(fabsf(mn), mx));
    }
}

}  // namespace

extern "C" {

// A prepared multi-tensor launch: the descriptors validated, classified and packed into kernel arguments once.
struct PlanStep {
    int mode = 0;              // 0: K1, 3: encode to storage codes, 4: decode (k_multi_flat<MODE>)
    bool batched;              // true: one k_multi_flat launch of `args`; false: one single-tensor call of `single`
    MultiArgs args;
    size_t shmem;
    fp8q_tensor_desc single;
};

}  // extern "C"

struct fp8q_multi_plan {
    std::vector<PlanStep> steps;
};

// step_of (optional, [n]): the index in plan.steps each descriptor landed in, -1 for an empty tensor (fp8q_multi_route)
static int plan_build(const fp8q_tensor_desc *descs, int n, fp8q_multi_plan &plan, int mode = 0, int *step_of = nullptr)
{
    if (n < 0 || (n > 0 && !descs)) return FP8Q_EINVAL;
    // validate everything first: nothing is built (or enqueued) if any descriptor is bad
    for (int i = 0; i < n; ++i) {
        const fp8q_tensor_desc &t = descs[i];
        if (t.C < 0 || t.inner < 0 || (t.n_maxval != 1 && t.n_maxval != t.C)) return FP8Q_EINVAL;
        QFmt f;
        if (int rc = make_fmt(t.mbits, t.n_bits, t.sign_bits, &f)) return rc;
        if (t.C > 0 && t.inner > 0 && (!t.x || !t.y || !t.maxval)) return FP8Q_EINVAL;
        // storage codes: one byte, at least one exponent bit (include/fp8q.h: FP8Q_EUNSUPPORTED otherwise)
        if (mode != 0 && (t.n_bits > 8 || t.n_bits - t.sign_bits - (int)f.M < 1)) return FP8Q_EUNSUPPORTED;
    }
    PlanStep cur;
    cur.mode = mode;
    cur.batched = true;
    cur.args.n = 0;
    cur.args.rpc_max = 0;
    cur.args.total_chunks = 0;
    cur.shmem = 0;
    size_t lut_max = 0;   // largest table area (rows x entries) any tensor of the current launch needs
    auto flush = [&]() {
        if (cur.args.n == 0) return;
        cur.shmem = (size_t)cur.args.rpc_max * 16 + lut_max;   // [chanlite[rpc_max] | tables]
        plan.steps.push_back(cur);
        cur.args.n = 0;
        cur.args.rpc_max = 0;
        cur.args.total_chunks = 0;
        cur.shmem = 0;
        lut_max = 0;
    };
    for (int i = 0; i < n; ++i) {
        const fp8q_tensor_desc &t = descs[i];
        if (step_of) step_of[i] = -1;
        if (t.C == 0 || t.inner == 0) continue;
        QFmt f;
        make_fmt(t.mbits, t.n_bits, t.sign_bits, &f);
        const bool per_channel = t.n_maxval != 1;
        const int64_t nelem = t.C * t.inner;
        const int64_t inner = per_channel ? t.inner : nelem;
        const int64_t rpc = per_channel ? flat_rpc(inner) : 1;
        const int64_t per_row = flat_per_row(f.pmax + 1);
        // 16-byte groups of fp32 on the value side, 4-byte groups of codes on the other
        const uintptr_t mis = mode == 3 ? (((uintptr_t)t.x & 15) | ((uintptr_t)t.y & 3))
                            : mode == 4 ? (((uintptr_t)t.x & 3) | ((uintptr_t)t.y & 15)) : (((uintptr_t)t.x | (uintptr_t)t.y) & 15);
        const bool batchable = mis == 0 && nelem >= 4 && nelem < (1ll << 31) &&
                               (!per_channel || (inner >= 4 && inner <= kMagicMaxDivisor)) &&
                               rpc * per_row <= 36 * 1024 && nelem * 4 < kNtBytes;
        if (!batchable) {   // unaligned, very short rows, or a tensor big enough to deserve its own launch
            flush();
            PlanStep one;
            one.mode = mode;
            one.batched = false;
            one.args.n = 0;
            one.args.rpc_max = 0;
            one.args.total_chunks = 0;
            one.shmem = 0;
            one.single = t;
            if (step_of) step_of[i] = (int)plan.steps.size();
            plan.steps.push_back(one);
            continue;
        }
        if (cur.args.n == kMultiMax) flush();
        if (step_of) step_of[i] = (int)plan.steps.size();   // where the next flush() puts `cur`
        MultiDesc &d = cur.args.d[cur.args.n++];
        d.x = t.x;
        d.y = t.y;
        d.maxval = t.maxval;
        d.nvec = nelem >> 2;
        d.tail = (int)(nelem & 3);
        d.single_row = per_channel ? 0 : 1;
        d.inner = per_channel ? (int)inner : 0;
        d.rpc = (int)rpc;
        d.magic = per_channel ? magic_of((int)inner) : 0u;
        d.chunk0 = cur.args.total_chunks;
        d.n_bits = t.n_bits;
        d.f = f;
        cur.args.total_chunks += (uint32_t)cdiv(d.nvec, kChunkGroups);
        // per table row: the channel constants (16 B) + pmax + 1 entries {s, 1/s}; every tensor of the launch uses the
        // same layout [chanlite[rpc_max] | tables], so size it for the largest of each
        if ((int)rpc > cur.args.rpc_max) cur.args.rpc_max = (int)rpc;
        const size_t need = (size_t)rpc * (size_t)(f.pmax + 1) * 8;
        if (need > lut_max) lut_max = need;
    }
    flush();
    return FP8Q_OK;
}

static int plan_launch(const fp8q_multi_plan &plan, hipStream_t st)
{
    for (const PlanStep &s : plan.steps) {
        if (s.batched) {
            // every block resident at once (4 per CU at 128 VGPRs): chunks grid-stride, a few per block
            static const int grid_env = [] {   // FP8Q_MULTI_GRID: block cap of the multi-tensor launch (tuning knob)
                const char *e = getenv("FP8Q_MULTI_GRID");
                const int v = e ? atoi(e) : 0;
                return v >= 1 ? v : 1024;
            }();
            const dim3 grid((unsigned)balanced_blocks(s.args.total_chunks, grid_env));
            dispatch<3, 4, 0>(s.mode, [&](auto MODE) {
                hipLaunchKernelGGL(k_multi_flat<MODE()>, grid, dim3(kBlock), s.shmem, st, s.args);
            });
            if (int rc = launch_rc()) return rc;
        } else {
            const fp8q_tensor_desc &t = s.single;
            int rc;
            if (s.mode == 3)
                rc = fp8q_encode_u8(t.x, reinterpret_cast<uint8_t *>(t.y), t.C, t.inner, t.maxval, t.n_maxval, t.mbits, t.n_bits,
                                    t.sign_bits, (fp8q_stream_t)st);
            else if (s.mode == 4)
                rc = fp8q_decode_u8(reinterpret_cast<const uint8_t *>(t.x), t.y, t.C, t.inner, t.maxval, t.n_maxval, t.mbits, t.n_bits,
                                    t.sign_bits, (fp8q_stream_t)st);
            else
                rc = fp8q_quantize_f32(t.x, t.y, t.C, t.inner, t.maxval, t.n_maxval, t.mbits, t.n_bits, t.sign_bits, (fp8q_stream_t)st);
            if (rc) return rc;
        }
    }
    return FP8Q_OK;
}

extern "C" {

int fp8q_multi_quantize_f32(const fp8q_tensor_desc *descs, int n, fp8q_stream_t stream)
{
    try {
        fp8q_multi_plan plan;
        if (int rc = plan_build(descs, n, plan)) return rc;
        return plan_launch(plan, (hipStream_t)stream);
    } catch (...) {
        return (int)hipErrorOutOfMemory;
    }
}

static int multi_codec(const fp8q_tensor_desc *descs, int n, fp8q_stream_t stream, int mode)
{
    try {
        fp8q_multi_plan plan;
        if (int rc = plan_build(descs, n, plan, mode)) return rc;
        return plan_launch(plan, (hipStream_t)stream);
    } catch (...) {
        return (int)hipErrorOutOfMemory;
    }
}

int fp8q_multi_encode_u8(const fp8q_tensor_desc *descs, int n, fp8q_stream_t stream) { return multi_codec(descs, n, stream, 3); }
int fp8q_multi_decode_u8(const fp8q_tensor_desc *descs, int n, fp8q_stream_t stream) { return multi_codec(descs, n, stream, 4); }

static int multi_minmax_then(const fp8q_tensor_desc *descs, float *const *maxval_out, int n, fp8q_stream_t stream, int mode);

int fp8q_multi_minmax_quantize_f32(const fp8q_tensor_desc *descs, float *const *maxval_out, int n, fp8q_stream_t stream)
{
    return multi_minmax_then(descs, maxval_out, n, stream, 0);
}

int fp8q_multi_minmax_encode_u8(const fp8q_tensor_desc *descs, float *const *maxval_out, int n, fp8q_stream_t stream)
{
    return multi_minmax_then(descs, maxval_out, n, stream, 3);
}

static int multi_minmax_then(const fp8q_tensor_desc *descs, float *const *maxval_out, int n, fp8q_stream_t stream, int mode)
{
    if (n < 0 || (n > 0 && (!descs || !maxval_out))) return FP8Q_EINVAL;
    for (int i = 0; i < n; ++i) {   // per-channel ranges only; nothing is enqueued if a descriptor is bad
        const fp8q_tensor_desc &t = descs[i];
        if (t.C < 0 || t.inner < 0 || t.n_maxval != t.C || t.C >= (1ll << 31) || t.inner >= (1ll << 31)) return FP8Q_EINVAL;
        QFmt f;
        if (int rc = make_fmt(t.mbits, t.n_bits, t.sign_bits, &f)) return rc;
        if (t.C > 0 && t.inner > 0 && (!t.x || !t.y || !maxval_out[i] || ((uintptr_t)t.x & 3))) return FP8Q_EINVAL;
        // the quantize launch reads the ranges where the range launch wrote them: descs[i].maxval names that buffer too
        // (or is NULL); an input range buffer elsewhere would be silently ignored -- refuse it
        if (t.maxval && t.maxval != maxval_out[i]) return FP8Q_EINVAL;
        // the codec's own constraints, checked HERE: the encode launch below would refuse the descriptor only after the
        // range launch had been enqueued (and had overwritten maxval_out)
        if (mode == 3 && (t.n_bits > 8 || t.n_bits - t.sign_bits - (int)f.M < 1)) return FP8Q_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    RowsArgs ra;
    ra.n = 0;
    ra.total_rows = 0;
    auto flush = [&]() -> int {
        if (ra.n == 0) return FP8Q_OK;
        hipLaunchKernelGGL(k_multi_rowmax, dim3((unsigned)cdiv(ra.total_rows, kBlock / 64)), dim3(kBlock), 0, st, ra);
        ra.n = 0;
        ra.total_rows = 0;
        return launch_rc();
    };
    for (int i = 0; i < n; ++i) {
        const fp8q_tensor_desc &t = descs[i];
        if (t.C == 0 || t.inner == 0) continue;
        if (ra.n == kMultiMax || (uint64_t)ra.total_rows + (uint64_t)t.C >= (1ull << 31))
            if (int rc = flush()) return rc;
        RowsDesc &d = ra.d[ra.n++];
        d.x = t.x;
        d.maxval = maxval_out[i];
        d.row_min = d.row_max = nullptr;
        d.inner = (int)t.inner;
        d.row0 = ra.total_rows;
        ra.total_rows += (uint32_t)t.C;
    }
    if (int rc = flush()) return rc;
    std::vector<fp8q_tensor_desc> q(descs, descs + n);
    for (int i = 0; i < n; ++i) q[i].maxval = maxval_out[i];
    // same stream: reads the ranges just written
    return mode == 3 ? fp8q_multi_encode_u8(q.data(), n, stream) : fp8q_multi_quantize_f32(q.data(), n, stream);
}

int fp8q_multi_route(const fp8q_tensor_desc *descs, int n, int mode, int *step_of, int *batched, int *n_steps)
{
    if ((mode != 0 && mode != 3 && mode != 4) || !n_steps || (n > 0 && (!step_of || !batched))) return FP8Q_EINVAL;
    try {
        fp8q_multi_plan plan;   // the plan the launch would build, not launched
        if (int rc = plan_build(descs, n, plan, mode, step_of)) return rc;
        for (int i = 0; i < n; ++i) batched[i] = step_of[i] < 0 ? -1 : (plan.steps[step_of[i]].batched ? 1 : 0);
        *n_steps = (int)plan.steps.size();
        return FP8Q_OK;
    } catch (...) {
        return (int)hipErrorOutOfMemory;
    }
}

int fp8q_multi_plan_create(const fp8q_tensor_desc *descs, int n, fp8q_multi_plan **plan_out)
{
    if (!plan_out) return FP8Q_EINVAL;
    *plan_out = nullptr;
    try {
        fp8q_multi_plan *plan = new fp8q_multi_plan();
        if (int rc = plan_build(descs, n, *plan)) {
            delete plan;
            return rc;
        }
        *plan_out = plan;
        return FP8Q_OK;
    } catch (...) {
        return (int)hipErrorOutOfMemory;
    }
}

int fp8q_multi_plan_launch(const fp8q_multi_plan *plan, fp8q_stream_t stream)
{
    if (!plan) return FP8Q_EINVAL;
    return plan_launch(*plan, (hipStream_t)stream);
}

int fp8q_multi_plan_launches(const fp8q_multi_plan *plan) { return plan ? (int)plan->steps.size() : FP8Q_EINVAL; }

void fp8q_multi_plan_destroy(fp8q_multi_plan *plan) { delete plan; }

}  // extern "C"
