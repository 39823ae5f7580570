// fp8q_select.hip -- percentile ranges (CurrentMinMaxEstimator(percentile=p)): exact selection of up to four order
// statistics per row of a contiguous [C, inner] float32 tensor, then one interpolation step -> lo[C], hi[C].
// Contract: include/fp8q.h "Percentile ranges" (ordering by the monotone key of the bit pattern, ranks in double on the
// host, interpolation in double with the difference rounded to float32 first, a NaN anywhere in a row -> NaN twice).
//
// A radix select over integer keys: no sort, no floating-point sums, every counter an integer -- the result is a function
// of the row's multiset of values and does not depend on the launch geometry or on the order of the atomics.
//   row-resident route (inner <= kResident): G lanes (a wave for rows up to kWaveRow, else the workgroup) own a whole row.
//       x is read from HBM once into LDS as keys; four 8-bit digit passes over the LDS copy narrow the four ranks' keys with
//       an LDS histogram per distinct live prefix; the interpolation runs in the same launch.
//   streaming route (longer rows, any C): three digit passes (11 + 11 + 10 key bits) as SEPARATE launches, k_sel_count<P>
//       (LDS histogram per workgroup of the keys whose higher digits match a live prefix -> the row's table in the workspace
//       with integer atomics, non-empty bins only) and k_sel_resolve<P> (table -> digit and remaining rank of each of the four
//       ranks; the last one interpolates).  Passes 2 and 3 re-read x.  No workgroup waits on another.
// Ranks that share a prefix (k and k + 1 nearly always do until the last digit) share one histogram: each keeps its own
// remaining rank inside it.  Keys equal to +0.0 (half of a post-ReLU activation) are counted in a register and added to their
// bin once per thread instead of serialising on one LDS address.
// No library primitive is used.
#include "fp8q_common.h"
#include "fp8q_percentile_ranks.h"

namespace {

constexpr int kResident = 8192;      // longest row of the row-resident route: 32 KiB of keys in LDS (+ 4 KiB of histograms)
constexpr int kWaveRow = 1024;       // rows up to here: one wave per row, four rows per workgroup
constexpr int kPiece = 4096;         // elements of one streaming step of a workgroup: 256 lanes x 16 B x 4 in flight
constexpr int kB1 = 11, kB2 = 11, kB3 = 10;           // digit widths of the streaming passes
constexpr int kTab1Words = (1 << kB1) + 8;            // pass-1 table of a row: 2048 bins, then the row's NaN count
constexpr int kTabNWords = 4 << kB2;                  // pass-2 / pass-3 tables of a row: four ranks x 2048 (x 1024) bins
constexpr int kStateWords = 16;                       // prefix[4], rank[4], pad[4], NaN count, pad[3]
constexpr uint32_t kZeroKey = 0x80000000u;            // key of +0.0

struct SelArgs {
    uint32_t k[4];       // ranks: k, k1 of q_lo, then k, k1 of q_hi
    double t_lo, t_hi;   // interpolation weights
};

struct SelWs {
    uint32_t *state;     // [C, kStateWords]
    uint32_t *tab1;      // [C, kTab1Words]
    uint32_t *tabn;      // [C, kTabNWords]
};

// -inf < ... < -0.0 < +0.0 < ... < +inf as unsigned integers (NaNs beyond both ends)
__device__ __forceinline__ uint32_t sel_key(uint32_t bits) { return (bits >> 31) ? ~bits : (bits | 0x80000000u); }
__device__ __forceinline__ float sel_unkey(uint32_t key) { return __uint_as_float((key >> 31) ? (key ^ 0x80000000u) : ~key); }
__device__ __forceinline__ bool sel_isnan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

// contract step 3: in double, the difference rounded to float32 first; one final rounding (no FMA: -ffp-contract=off)
__device__ __forceinline__ float sel_interp(uint32_t ka, uint32_t kb, double t)
{
    const float a = sel_unkey(ka), b = sel_unkey(kb);
    const float df = b - a;
    const double d = (double)df;
    const double v = t < 0.5 ? (double)a + d * t : (double)b - d * (1.0 - t);
    return (float)v;
}

__device__ __forceinline__ void sel_store(const uint32_t *key, bool nan, const SelArgs &a, int64_t row, float *lo, float *hi)
{
    const float qn = __builtin_nanf("");
    lo[row] = nan ? qn : sel_interp(key[0], key[1], a.t_lo);
    hi[row] = nan ? qn : sel_interp(key[2], key[3], a.t_hi);
}

// One wave, a histogram h of 64 * PER bins (LDS or global), a rank r below the histogram's total: the bin that holds the
// element of rank r and r's rank inside that bin, in every lane.  (r beyond the total -- never, the ranks are below the
// row length -- gives the last bin: every index derived from the result stays inside its table.)
template <int PER>
__device__ __forceinline__ void wave_find(const uint32_t *h, uint32_t r, uint32_t &digit, uint32_t &rem)
{
    const int lane = threadIdx.x & 63;
    uint32_t c[PER], s = 0u;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        c[q] = h[lane * PER + q];
        s += c[q];
    }
    uint32_t incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    uint32_t acc = incl - s;
    const bool mine = r >= acc && r < incl;
    uint32_t d = 64u * PER - 1u, rm = 0u;
    if (mine) {
        bool found = false;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (!found && r < acc + c[q]) {
                d = (uint32_t)(lane * PER + q);
                rm = r - acc;
                found = true;
            }
            acc += c[q];
        }
    }
    const unsigned long long who = __ballot(mine);
    const int src = who ? __builtin_ctzll(who) : 63;
    digit = __shfl(d, src, 64);
    rem = __shfl(rm, src, 64);
}

// rank j counts into its own histogram only if no earlier rank has the same prefix (that one's histogram serves both)
__device__ __forceinline__ int sel_rep(const uint32_t (&p)[4], int j)
{
    int r = j;
#pragma unroll
    for (int i = 3; i >= 0; --i)
        if (i < j && p[i] == p[j]) r = i;
    return r;
}

// ---- row-resident route -------------------------------------------------------------------------------------------------
// G lanes per row, 256 / G rows per workgroup and step, rows handed out grid-stride.  Every barrier is reached by the whole
// workgroup the same number of times: the trip counts depend on C and the grid only.
template <int G, bool NT>
__global__ void __launch_bounds__(kBlock)
k_sel_resident(const float *__restrict__ x, int64_t C, int inner, SelArgs a, float *__restrict__ lo, float *__restrict__ hi)
{
    constexpr int RPB = kBlock / G;                              // rows per workgroup and step
    constexpr int CAP = G == 64 ? kWaveRow : kResident;          // keys per row in LDS
    constexpr int WPG = G / 64;                                  // waves per row
    __shared__ uint32_t s_key[RPB * CAP];
    __shared__ uint32_t s_hist[RPB][4][256];
    __shared__ uint32_t s_pre[RPB][4], s_rank[RPB][4], s_nan[RPB];
    const int tid = threadIdx.x, grp = tid / G, sub = tid % G, wig = sub >> 6;
    uint32_t *keys = s_key + grp * CAP;
    uint32_t *hist = &s_hist[grp][0][0];

    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < C; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t row = r0 + grp;
        const bool active = row < C;
        const int n = active ? inner : 0;
        for (int i = sub; i < 4 * 256; i += G) hist[i] = 0u;
        if (sub < 4) {
            s_pre[grp][sub] = 0u;
            s_rank[grp][sub] = a.k[sub];
        }
        if (sub == 0) s_nan[grp] = 0u;
        __syncthreads();
        // the row, once: scalar head up to the first 16-byte boundary, aligned 16-byte loads, scalar tail
        if (active) {
            const float *xr = x + row * inner;
            int head = (int)((4 - (((uintptr_t)xr >> 2) & 3)) & 3);
            if (head > n) head = n;
            const int nvec = (n - head) >> 2, bend = head + (nvec << 2);
            uint32_t nan = 0u;
            if (sub < head) {
                const uint32_t b = __float_as_uint(xr[sub]);
                nan |= sel_isnan(b);
                keys[sub] = sel_key(b);
            }
            const vf4 *xv = reinterpret_cast<const vf4 *>(xr + head);
            int i = sub;
            for (; i + 3 * G < nvec; i += 4 * G) {                // four 16-byte loads in flight
                vf4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = ld16<NT>(xv + i + u * G);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t b0 = __float_as_uint(v[u].x), b1 = __float_as_uint(v[u].y), b2 = __float_as_uint(v[u].z),
                                   b3 = __float_as_uint(v[u].w);
                    nan |= sel_isnan(b0) | sel_isnan(b1) | sel_isnan(b2) | sel_isnan(b3);
                    uint32_t *k = keys + head + 4 * (i + u * G);
                    k[0] = sel_key(b0);
                    k[1] = sel_key(b1);
                    k[2] = sel_key(b2);
                    k[3] = sel_key(b3);
                }
            }
            for (; i < nvec; i += G) {
                const vf4 v = ld16<NT>(xv + i);
                const uint32_t b0 = __float_as_uint(v.x), b1 = __float_as_uint(v.y), b2 = __float_as_uint(v.z), b3 = __float_as_uint(v.w);
                nan |= sel_isnan(b0) | sel_isnan(b1) | sel_isnan(b2) | sel_isnan(b3);
                uint32_t *k = keys + head + 4 * i;
                k[0] = sel_key(b0);
                k[1] = sel_key(b1);
                k[2] = sel_key(b2);
                k[3] = sel_key(b3);
            }
            for (int j = bend + sub; j < n; j += G) {
                const uint32_t b = __float_as_uint(xr[j]);
                nan |= sel_isnan(b);
                keys[j] = sel_key(b);
            }
            if (nan) atomicOr(&s_nan[grp], 1u);
        }
        __syncthreads();
        // four digit passes over the LDS copy, most significant first
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            uint32_t pre[4];
            bool live[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) pre[j] = s_pre[grp][j];
#pragma unroll
            for (int j = 0; j < 4; ++j) live[j] = sel_rep(pre, j) == j;
            for (int i = sub; i < n; i += G) {
                const uint32_t key = keys[i];
                const uint32_t hi_bits = pass ? key >> (shift + 8) : 0u, d = (key >> shift) & 255u;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (live[j] && hi_bits == pre[j]) atomicAdd(&hist[j * 256 + d], 1u);
            }
            __syncthreads();
            // a wave per rank (workgroup-owned rows: wave j <-> rank j; wave-owned rows: the wave takes all four)
            uint32_t dg[4 / WPG], rm[4 / WPG];
#pragma unroll
            for (int q = 0; q < 4 / WPG; ++q) {
                const int j = WPG == 4 ? wig : q;
                wave_find<4>(hist + sel_rep(pre, j) * 256, s_rank[grp][j], dg[q], rm[q]);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4 / WPG; ++q) {
                const int j = WPG == 4 ? wig : q;
                if ((sub & 63) == 0) {
                    s_pre[grp][j] = (pre[j] << 8) | dg[q];
                    s_rank[grp][j] = rm[q];
                }
            }
            for (int i = sub; i < 4 * 256; i += G) hist[i] = 0u;
            __syncthreads();
        }
        if (active && sub == 0) {
            const uint32_t key[4] = {s_pre[grp][0], s_pre[grp][1], s_pre[grp][2], s_pre[grp][3]};
            sel_store(key, s_nan[grp] != 0u, a, row, lo, hi);
        }
        __syncthreads();
    }
}

// ---- streaming route ------------------------------------------------------------------------------------------------------
// Workgroup (row, split) counts the pieces [split * pps, (split + 1) * pps) of its row.  A piece is kPiece elements from the
// row's first 16-byte boundary on; the <= 3 elements in front of the boundary belong to piece 0, the elements behind the
// last whole vector are read one by one.
template <int PASS, bool NT>
__global__ void __launch_bounds__(kBlock)
k_sel_count(const float *__restrict__ x, int64_t inner, int nsplit, int64_t pps, int64_t npr, SelWs w)
{
    constexpr int NB = PASS == 3 ? (1 << kB3) : (1 << kB2);      // (kB1 == kB2)
    constexpr int NTAB = PASS == 1 ? 1 : 4;
    constexpr int LOW = PASS == 1 ? kB2 + kB3 : (PASS == 2 ? kB3 : 0);      // key bits below this pass's digit
    __shared__ uint32_t s_hist[NTAB * NB + 1];                   // (+ the NaN count of pass 1)
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x / nsplit;
    const int split = (int)(blockIdx.x - row * nsplit);
    const float *xr = x + row * inner;
    int64_t head = (int64_t)((4 - (((uintptr_t)xr >> 2) & 3)) & 3);
    if (head > inner) head = inner;

    uint32_t pre[4] = {0u, 0u, 0u, 0u};
    bool live[4] = {true, false, false, false};
    if (PASS > 1) {
        const uint32_t *st = w.state + row * kStateWords;
#pragma unroll
        for (int j = 0; j < 4; ++j) pre[j] = st[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) live[j] = sel_rep(pre, j) == j;
    }
    for (int i = tid; i < NTAB * NB + 1; i += kBlock) s_hist[i] = 0u;
    __syncthreads();

    uint32_t nz = 0u, nnan = 0u;
    auto count = [&](uint32_t bits) {
        const uint32_t key = sel_key(bits);
        if (PASS == 1) nnan += sel_isnan(bits) ? 1u : 0u;
        if (key == kZeroKey) {
            ++nz;
            return;
        }
        const uint32_t d = (key >> LOW) & (uint32_t)(NB - 1);
        if (PASS == 1) {
            atomicAdd(&s_hist[d], 1u);
        } else {
            const uint32_t hi_bits = key >> (LOW + (PASS == 2 ? kB2 : kB3));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live[j] && hi_bits == pre[j]) atomicAdd(&s_hist[j * NB + d], 1u);
        }
    };

    const int64_t p0 = (int64_t)split * pps, p1 = min(p0 + pps, npr);
    if (p0 == 0 && tid < head) count(__float_as_uint(xr[tid]));
    for (int64_t p = p0; p < p1; ++p) {
        const int64_t base = head + p * kPiece;
        if (base + kPiece <= inner) {
            vf4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = ld16<NT>(reinterpret_cast<const vf4 *>(xr + base) + u * kBlock + tid);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                count(__float_as_uint(v[u].x));
                count(__float_as_uint(v[u].y));
                count(__float_as_uint(v[u].z));
                count(__float_as_uint(v[u].w));
            }
        } else {
#pragma unroll 1
            for (int u = 0; u < 4; ++u) {
                const int64_t i = base + (int64_t)(u * kBlock + tid) * 4;
                if (i + 4 <= inner) {
                    const vf4 v = ld16<NT>(reinterpret_cast<const vf4 *>(xr + i));
                    count(__float_as_uint(v.x));
                    count(__float_as_uint(v.y));
                    count(__float_as_uint(v.z));
                    count(__float_as_uint(v.w));
                } else {
                    for (int64_t e = i; e < inner; ++e) count(__float_as_uint(xr[e]));
                }
            }
        }
    }
    // the +0.0 keys of this thread, once
    if (nz) {
        if (PASS == 1) {
            atomicAdd(&s_hist[kZeroKey >> LOW], nz);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live[j] && pre[j] == (kZeroKey >> (LOW + (PASS == 2 ? kB2 : kB3)))) atomicAdd(&s_hist[j * NB], nz);
        }
    }
    if (PASS == 1 && nnan) atomicAdd(&s_hist[NB], nnan);
    __syncthreads();
    uint32_t *tab = PASS == 1 ? w.tab1 + row * kTab1Words : w.tabn + row * kTabNWords;
    for (int i = tid; i < NTAB * NB + (PASS == 1 ? 1 : 0); i += kBlock) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&tab[i], v);
    }
}

// The tiny step between the passes: a workgroup per row (grid-stride), wave j <-> rank j.  Pass 1 also keeps the row's NaN
// count, pass 2 clears the tables for pass 3, pass 3 interpolates.
template <int PASS>
__global__ void __launch_bounds__(kBlock)
k_sel_resolve(int64_t C, SelArgs a, SelWs w, float *__restrict__ lo, float *__restrict__ hi)
{
    constexpr int NB = PASS == 3 ? (1 << kB3) : (1 << kB2);
    constexpr int BITS = PASS == 3 ? kB3 : kB2;
    __shared__ uint32_t s_pre[4], s_rank[4];
    const int tid = threadIdx.x, j = tid >> 6;
    for (int64_t row = blockIdx.x; row < C; row += gridDim.x) {
        uint32_t *st = w.state + row * kStateWords;
        uint32_t pre[4] = {0u, 0u, 0u, 0u};
        uint32_t rank = a.k[j];
        if (PASS > 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) pre[i] = st[i];
            rank = st[4 + j];
        }
        const uint32_t *tab = PASS == 1 ? w.tab1 + row * kTab1Words : w.tabn + row * kTabNWords + sel_rep(pre, j) * NB;
        uint32_t dg, rm;
        wave_find<NB / 64>(tab, rank, dg, rm);
        if ((tid & 63) == 0) {
            s_pre[j] = (pre[j] << BITS) | dg;
            s_rank[j] = rm;
        }
        __syncthreads();                           // every wave has read the state and its table
        if (tid < 4) {
            st[tid] = s_pre[tid];
            st[4 + tid] = s_rank[tid];
        }
        if (PASS == 1 && tid == 0) st[12] = w.tab1[row * kTab1Words + NB];
        if (PASS == 2)
            for (int i = tid; i < kTabNWords; i += kBlock) w.tabn[row * kTabNWords + i] = 0u;
        if (PASS == 3 && tid == 0) {
            const uint32_t key[4] = {s_pre[0], s_pre[1], s_pre[2], s_pre[3]};
            sel_store(key, st[12] != 0u, a, row, lo, hi);
        }
        __syncthreads();                           // s_pre / s_rank are free again
    }
}

constexpr size_t kRowWsBytes = 4 * (size_t)(kStateWords + kTab1Words + kTabNWords);

int launch_resident(const float *x, int64_t C, int inner, const SelArgs &a, float *lo, float *hi, hipStream_t st)
{
    const bool nt = C * (int64_t)inner * 4 >= kNtBytes;
    const bool wave = inner <= kWaveRow;
    const int64_t steps = wave ? cdiv(C, 4) : C;
    const dim3 g((unsigned)balanced_blocks(steps, 4 * 256)), b(kBlock);
    dispatch<false, true>(nt, [&](auto NT) {
        if (wave)
            hipLaunchKernelGGL((k_sel_resident<64, NT()>), g, b, 0, st, x, C, inner, a, lo, hi);
        else
            hipLaunchKernelGGL((k_sel_resident<kBlock, NT()>), g, b, 0, st, x, C, inner, a, lo, hi);
    });
    return launch_rc();
}

int launch_streaming(const float *x, int64_t C, int64_t inner, const SelArgs &a, float *lo, float *hi, void *ws, hipStream_t st)
{
    SelWs w;
    w.state = static_cast<uint32_t *>(ws);
    w.tab1 = w.state + C * kStateWords;
    w.tabn = w.tab1 + C * kTab1Words;
    int rc = hip_rc(hipMemsetAsync(ws, 0, (size_t)C * kRowWsBytes, st));
    if (rc != FP8Q_OK) return rc;
    const bool nt = C * inner * 4 >= kNtBytes;
    const int64_t npr = cdiv(inner, kPiece);
    int64_t nsplit = cdiv(1024, C);                         // ~1024 workgroups when there are few rows, one per row otherwise
    if (nsplit > npr) nsplit = npr;
    const int64_t pps = cdiv(npr, nsplit);
    nsplit = cdiv(npr, pps);
    const dim3 g((unsigned)(C * nsplit)), b(kBlock), gr((unsigned)(C < 2048 ? C : 2048));
    dispatch<false, true>(nt, [&](auto NT) {
        hipLaunchKernelGGL((k_sel_count<1, NT()>), g, b, 0, st, x, inner, (int)nsplit, pps, npr, w);
        hipLaunchKernelGGL((k_sel_resolve<1>), gr, b, 0, st, C, a, w, lo, hi);
        hipLaunchKernelGGL((k_sel_count<2, NT()>), g, b, 0, st, x, inner, (int)nsplit, pps, npr, w);
        hipLaunchKernelGGL((k_sel_resolve<2>), gr, b, 0, st, C, a, w, lo, hi);
        hipLaunchKernelGGL((k_sel_count<3, NT()>), g, b, 0, st, x, inner, (int)nsplit, pps, npr, w);
        hipLaunchKernelGGL((k_sel_resolve<3>), gr, b, 0, st, C, a, w, lo, hi);
    });
    return launch_rc();
}

}  // namespace

extern "C" int64_t fp8q_percentile_resident_max_inner(void) { return kResident; }

extern "C" size_t fp8q_percentile_workspace_bytes(int64_t C, int64_t inner)
{
    if (C < 1 || inner <= kResident) return 0;
    return (size_t)C * kRowWsBytes;
}

extern "C" int fp8q_percentile_f32(const float *x, int64_t C, int64_t inner, double pct, float *lo, float *hi, void *ws,
                                   size_t ws_bytes, fp8q_stream_t stream)
{
    if (!x || !lo || !hi || C < 1 || inner < 1) return FP8Q_EINVAL;
    if (!(pct >= 0.0 && pct <= 100.0)) return FP8Q_EINVAL;                        // (a NaN fails both comparisons)
    if (((uintptr_t)x | (uintptr_t)lo | (uintptr_t)hi) & 3) return FP8Q_EINVAL;
    const bool resident = inner <= kResident;
    if (!resident) {
        if (!ws || ((uintptr_t)ws & 7) || ws_bytes < fp8q_percentile_workspace_bytes(C, inner)) return FP8Q_EINVAL;
        // ranks and counts are 32-bit words, a launch has fewer than 2^31 workgroups
        if (inner > (int64_t)0xffffffffll || C > ((int64_t)1 << 30)) return FP8Q_EUNSUPPORTED;
    }
    SelArgs a;
    int64_t k, k1;
    fp8q_percentile_rank(pct / 100.0, inner, &k, &k1, &a.t_lo);
    a.k[0] = (uint32_t)k;
    a.k[1] = (uint32_t)k1;
    fp8q_percentile_rank((100.0 - pct) / 100.0, inner, &k, &k1, &a.t_hi);
    a.k[2] = (uint32_t)k;
    a.k[3] = (uint32_t)k1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return resident ? launch_resident(x, C, (int)inner, a, lo, hi, st) : launch_streaming(x, C, inner, a, lo, hi, ws, st);
}
