// fp8q_mxtq.h -- what the kernels with the MX blocks along dim 0 share (fp8q_mx_t.hip, fp8q_mx_had_t.hip): the tile of 128 rows
// x 64 columns, the layout of its transposed codes in LDS, the argument block and the stores of those codes.  fp8q_mx_t.hip's
// header explains the geometry and the bank arithmetic.  Internal linkage, as fp8q_common.h.
#pragma once
#include "fp8q_common.h"
#include "fp8q_io.h"
#include "fp8q_mxq.h"

namespace {

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

}  // namespace
