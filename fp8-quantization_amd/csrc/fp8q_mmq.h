// fp8q_mmq.h -- what the matrix-core products share (fp8q_mx_mm.hip: MX operands under E8M0 block scales, and its small-M
// kernel fp8q_mx_mm_skinny.hip, which takes the chunk loads, the stores, the load width and the MX format table, and its
// grouped form fp8q_mx_mm_grouped.hip, which takes everything and a 32-row panel besides; fp8q_ocp_block_mm.hip: hardware FP8 under float32 tile scales): the 128-row tile and its 256 lanes, an operand's panel of one
// K step in LDS with its bank-conflict-free layout, the chunk loads that narrow with the operand's alignment, the fragment a
// lane hands to v_mfma_*_16x16x128_f8f6f4, the masked stores of a lane's four results, and the one host rule for the load
// width.  fp8q_mx_mm.hip's header has the instruction's operand and result layouts and the bank arithmetic.  Which bytes of a
// row a step may read (the K tail) and the scales are each unit's own.  Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_half.h"

namespace {

constexpr int kMmTile = 128;     // rows of either operand under one workgroup
constexpr int kMmBlock = 256;

typedef int i8v __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));

// ---- the MX formats, for the two MX products (fp8q_mx_mm.hip, fp8q_mx_mm_skinny.hip) ----
constexpr int kMmScaleOne = 127; // the E8M0 byte of 2^0: what masked rows and blocks carry

// FP8Q_MX_* -> the instruction's format number and the element width
template <int F> struct MmFmt;
template <> struct MmFmt<FP8Q_MX_E4M3FN> { static constexpr int hw = 0, bits = 8; };
template <> struct MmFmt<FP8Q_MX_E5M2> { static constexpr int hw = 1, bits = 8; };
template <> struct MmFmt<FP8Q_MX_E2M3> { static constexpr int hw = 2, bits = 6; };
template <> struct MmFmt<FP8Q_MX_E3M2> { static constexpr int hw = 3, bits = 6; };
template <> struct MmFmt<FP8Q_MX_E2M1> { static constexpr int hw = 4, bits = 4; };

// one operand's panel of a K step in LDS (fp8q_mx_mm.hip's header has the bank arithmetic).  ROWS is 128 everywhere but in
// fp8q_mx_mm_grouped.hip's 32-row X panel, whose 256 / 192 / 128 chunks leave lanes idle (kWhole false): chunk_at depends on
// the row alone, so the layout and its bank arithmetic hold for any multiple of 16 rows.
template <int BITS, int ROWS = kMmTile>
struct MmPanel {
    static constexpr int kBlockBytes = 4 * BITS;            // one MX block: 32 / 24 / 16
    static constexpr int kStepBytes = 4 * kBlockBytes;      // a row's four blocks: 128 / 96 / 64
    static constexpr int kChunks = kStepBytes / 16;         // 8 / 6 / 4
    static constexpr bool kSwizzle = BITS != 6;
    static constexpr int kPitch = kSwizzle ? kStepBytes : kStepBytes + 16;
    static constexpr int kBytes = ROWS * kPitch;
    static constexpr int kCount = ROWS * kChunks;                           // the panel's chunks
    static constexpr int kPerLane = (kCount + kMmBlock - 1) / kMmBlock;     // 128 rows: 4 / 3 / 2 chunks per lane
    static constexpr bool kWhole = kCount % kMmBlock == 0;                  // every lane has kPerLane chunks
    static __device__ __forceinline__ int chunk_at(int row, int c)
    {
        if constexpr (kSwizzle) return row * kPitch + 16 * (c ^ ((row / (256 / kStepBytes)) % kChunks));
        else return row * kPitch + 16 * c;
    }
};

// the first `nvalid` bytes at p, zero-extended to 16, by loads of w bytes; p is w-aligned and nvalid a multiple of w (the MX
// product asks for 0, 8 or 16)
__device__ __forceinline__ u4v mm_load_chunk(const uint8_t *p, int nvalid, int w)
{
    u4v v = {0u, 0u, 0u, 0u};
    if (nvalid == 0) return v;
    if (w == 16 && nvalid == 16) return *reinterpret_cast<const u4v *>(p);
    if (w >= 8) {
        const u2v lo = *reinterpret_cast<const u2v *>(p);
        v.x = lo.x;
        v.y = lo.y;
        if (nvalid == 16) {
            const u2v hi = *reinterpret_cast<const u2v *>(p + 8);
            v.z = hi.x;
            v.w = hi.y;
        }
        return v;
    }
    uint32_t d[4] = {0u, 0u, 0u, 0u};
    if (w == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * i < nvalid) d[i] = *reinterpret_cast<const uint32_t *>(p + 4 * i);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i < nvalid) d[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
    v.x = d[0];
    v.y = d[1];
    v.z = d[2];
    v.w = d[3];
    return v;
}

template <class P>
__device__ __forceinline__ void mm_store_panel(uint8_t *s, const u4v (&g)[P::kPerLane], int tid)
{
#pragma unroll
    for (int j = 0; j < P::kPerLane; ++j) {
        const int q = tid + j * kMmBlock;
        if (!P::kWhole && q >= P::kCount) continue;
        *reinterpret_cast<u4v *>(s + P::chunk_at(q / P::kChunks, q % P::kChunks)) = g[j];
    }
}

// a lane's operand of panel row `row` (FP6 / FP4: block g; FP8: the two 16-byte runs of fp8q_mx_mm.hip's header), the registers
// past the format's 8 / 6 / 4 unused by the instruction
template <class P>
__device__ __forceinline__ i8v mm_read_frag(const uint8_t *s, int row, int g)
{
    i8v f = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (P::kBlockBytes == 32) {
        const u4v lo = *reinterpret_cast<const u4v *>(s + P::chunk_at(row, g));          // K [16 g, 16 g + 16) of the step
        const u4v hi = *reinterpret_cast<const u4v *>(s + P::chunk_at(row, 4 + g));      // K [64 + 16 g, 64 + 16 g + 16)
        f[0] = (int)lo.x, f[1] = (int)lo.y, f[2] = (int)lo.z, f[3] = (int)lo.w;
        f[4] = (int)hi.x, f[5] = (int)hi.y, f[6] = (int)hi.z, f[7] = (int)hi.w;
    } else if constexpr (P::kBlockBytes == 16) {
        const u4v lo = *reinterpret_cast<const u4v *>(s + P::chunk_at(row, g));
        f[0] = (int)lo.x, f[1] = (int)lo.y, f[2] = (int)lo.z, f[3] = (int)lo.w;
    } else {
        const u2v *p = reinterpret_cast<const u2v *>(s + row * P::kPitch + 24 * g);
        const u2v a = p[0], b = p[1], c = p[2];
        f[0] = (int)a.x, f[1] = (int)a.y, f[2] = (int)b.x, f[3] = (int)b.y, f[4] = (int)c.x, f[5] = (int)c.y;
    }
    return f;
}

// y[e .. e + 3] (the first `n` of them) = v, a half type rounded once; vec: one store of the four
template <class T>
__device__ __forceinline__ void mm_store4_half(uint16_t *y, int64_t e, const f4v v, int n, bool vec)
{
    if (vec) {
        u2v h;
        h.x = T::narrow2(v[0], v[1]);
        h.y = T::narrow2(v[2], v[3]);
        *reinterpret_cast<u2v *>(y + e) = h;
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < n) y[e + r] = T::narrow1(v[r]);
}

__device__ __forceinline__ void mm_store4(void *y, int y_type, int64_t e, const f4v v, int n, bool vec)
{
    if (y_type == FP8Q_DT_F16) return mm_store4_half<F16>(static_cast<uint16_t *>(y), e, v, n, vec);
    if (y_type == FP8Q_DT_BF16) return mm_store4_half<BF16>(static_cast<uint16_t *>(y), e, v, n, vec);
    float *yf = static_cast<float *>(y);
    if (vec) {
        *reinterpret_cast<f4v *>(yf + e) = v;
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < n) yf[e + r] = v[r];
}

// ---- host side ----
// the five MX element formats and the bytes of one block of 32 elements
inline bool mm_fmt_known(int f)
{
    return f == FP8Q_MX_E4M3FN || f == FP8Q_MX_E5M2 || f == FP8Q_MX_E2M1 || f == FP8Q_MX_E2M3 || f == FP8Q_MX_E3M2;
}

inline int mm_block_bytes(int f) { return f == FP8Q_MX_E2M1 ? 16 : ((f == FP8Q_MX_E2M3 || f == FP8Q_MX_E3M2) ? 24 : 32); }

// The one place that decides how a codes operand is loaded: the widest of 16, 8, 4 bytes that divides both the pointer and the
// row pitch (so that every row, and every 16-byte chunk of it, starts aligned), else single bytes.
inline int mm_load_width(const void *codes, int64_t pitch)
{
    for (int w = 16; w >= 4; w >>= 1)
        if ((uintptr_t)codes % (uintptr_t)w == 0 && pitch % w == 0) return w;
    return 1;
}

}  // namespace
