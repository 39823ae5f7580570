// fp8q_bwd.h -- what the two backward translation units (fp8q_grad.hip: the FP quantizer, fp8q_intgrad.hip: the uniform
// quantizers) share: the fixed-order fp64 block sums and the launch geometry of the streaming pass.  Internal linkage, as
// fp8q_common.h.
#pragma once
#include "fp8q_common.h"

namespace {

constexpr int kShortMaxInner = 2048;     // rows up to here: lane groups (k_bwd_short)
constexpr int64_t kBwdMaxItems = 16384;  // most blocks (= partial sums) of a launch unless there are more rows than that

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// fixed-order sum over the block; the result is valid in thread 0 (call uniformly)
__device__ __forceinline__ void block_sum2(double &a, double &b)
{
    static_assert(kBlock == 256, "block_sum2 combines exactly four waves");
    __shared__ double s_a[kBlock / 64], s_b[kBlock / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    a = wave_sum(a);
    b = wave_sum(b);
    __syncthreads();          // (a previous call's s_a / s_b are no longer read)
    if (lane == 0) {
        s_a[wave] = a;
        s_b[wave] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((s_a[0] + s_a[1]) + s_a[2]) + s_a[3];
        b = ((s_b[0] + s_b[1]) + s_b[2]) + s_b[3];
    }
}

// launch geometry, a pure function of the shape (the workspace size follows from it)
struct BwdPlan {
    bool shortrows;
    int G;           // k_bwd_short: lanes per row
    int64_t C, inner;
    int64_t nsplit;  // k_bwd_rows: blocks per row
    int64_t blocks;
    int U;
    bool nt;
};

BwdPlan bwd_plan(int64_t C, int64_t inner, int64_t n_maxval)
{
    BwdPlan p = {};
    const bool per_channel = n_maxval != 1;
    if (!per_channel) {
        inner *= C;
        C = 1;
    }
    p.C = C;
    p.inner = inner;
    p.nt = C * inner * 4 >= kNtBytes;
    p.U = kUnroll;
    if (per_channel && inner <= kShortMaxInner) {
        p.shortrows = true;
        int G = 1;
        while (G < 64 && (int64_t)G * 24 < inner) G <<= 1;
        p.G = G;
        p.blocks = balanced_blocks(cdiv(C, kBlock / G), kBwdMaxItems);
        return p;
    }
    const bool small = C == 1 && inner < ((int64_t)8 << 20);       // cache-sized per-tensor calls: 4 KiB pieces, more blocks
    if (small) p.U = 1;
    const int64_t pieces = inner / (4 * kBlock * p.U) > 0 ? inner / (4 * kBlock * p.U) : 1;
    const int64_t total_cap = p.nt ? kBwdMaxItems : kTargetBlocks;
    const int64_t cap = total_cap / C > 0 ? total_cap / C : 1;
    p.nsplit = balanced_blocks(pieces, cap);
    p.blocks = C * p.nsplit;
    return p;
}

// an upper bound of the plan's blocks that grows with C, inner and n_maxval
int64_t bwd_items_bound(int64_t C, int64_t inner, int64_t n_maxval)
{
    const int64_t rows = n_maxval == 1 ? 1 : C;
    const int64_t pieces = cdiv(C * inner, 4 * kBlock);
    const int64_t capped = pieces < kBwdMaxItems ? pieces : kBwdMaxItems;
    return rows > capped ? rows : capped;
}

}  // namespace
