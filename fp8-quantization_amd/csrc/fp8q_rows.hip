// fp8q_rows.hip -- the short-row per-channel kernels of the quantize / min-max family (file map: fp8q_quant.hip), their
// launchers and the entry points that only choose among them.  k_rows_reg has a unit of its own (fp8q_rowsreg.hip).
#include "fp8q_rows.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Short rows, register-streamed: k_rows_direct (inner <= kDirectMaxInner).
// G lanes own one row: every element a lane touches belongs to ONE channel, so the channel
// constants / table pointer are loaded once per row and the inner loop is the per-tensor one.
// Rows start at arbitrary 4-byte offsets: lanes use 16-byte accesses at 4-byte alignment (one
// dwordx4 each); the G lanes of a row cover G*16 contiguous bytes per instruction.
// A block takes R rows per iteration; LDS holds only the tables of those rows:
//   pass A (MODE 1, 2) row min/max straight from global, G-lane shuffle reduction
//   tables            make_chan (thread j <-> row j), then {s, 1/s} entries over all threads
//   pass B            quantize the R rows as one flat contiguous range (coalesced 16-byte I/O);
//                     in MODE 1 this re-reads the rows, which are L2-resident
// Dynamic LDS: float rowmv[R4] | float4 patch[R] | Chan chans[R] | float2 lut[R * lut_stride]
// ---------------------------------------------------------------------------------------------
template <int MODE, bool LUT, bool NT>
__global__ void __launch_bounds__(kBlock, 4)   // <= 128 VGPRs: 4 blocks of 256 per CU
k_rows_direct(const float *__restrict__ x, float *__restrict__ y, int64_t C,
              const float *__restrict__ maxval, float *row_min, float *row_max, float *maxval_out,
              QFmt f, TileArgs a, FoldArgs fa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Rmax = a.rows;
    float *rowmv = reinterpret_cast<float *>(smem);
    float4 *patch = reinterpret_cast<float4 *>(rowmv + ((Rmax + 3) & ~3));
    Chan *chans = reinterpret_cast<Chan *>(patch + Rmax);
    float2 *lut = reinterpret_cast<float2 *>(chans + Rmax);
    const int tid = threadIdx.x;
    constexpr int BS = kBlock;
    const int G = a.group, rpp = BS / G;
    const int sub = tid & (G - 1), slot = tid / G;
    const int inner = a.inner, inner4 = inner & ~3;
    const float pmaxf = (float)f.pmax;
    // log2/exp2 tables: staged in LDS for 256-thread blocks; single-wave blocks read them through L1
    __shared__ double ftab_lds[kFastTabSize];
    const double *ftab = ftab_lds;
    if (MODE != kModeMinMax)
        for (int i = threadIdx.x; i < kFastTabSize; i += BS) ftab_lds[i] = kFastTab[i];

    for (int64_t r0 = (int64_t)blockIdx.x * Rmax; r0 < C; r0 += (int64_t)gridDim.x * Rmax) {
        const int R = (int)((C - r0) < Rmax ? (C - r0) : Rmax);
        // geometry of pass B (the R rows as one flat range) -- needed early for the prefetch
        const int n = R * inner;
        const float *xt = x + r0 * inner;
        float *yt = y + r0 * inner;
        int head = a.coaligned ? (int)((4 - (((uintptr_t)xt >> 2) & 3)) & 3) : 0;
        if (head > n || inner < 4) head = n;          // rows shorter than a group: all scalar
        const int nvec = (n - head) >> 2;
        const int bend = head + (nvec << 2);
        constexpr int U = 4;   // four 16-byte loads in flight per lane
        // (prefetching the first U loads before the table phase was measured: +25 VGPRs, one wave
        // per SIMD less, -8 %: not done)
        __syncthreads();   // tables of the previous iteration are no longer read (and ftab is staged)
        if (MODE != kModeQuant) {
            for (int rb = 0; rb < R; rb += rpp) {
                const int r = rb + slot;
                MinMax m;
                mm_init(m);
                if (r < R) {
                    const float *xr = x + (r0 + r) * inner;
                    int i = sub * 4;
                    for (; i + 3 * G * 4 < inner4; i += G * 16) {   // four 16-byte loads in flight
                        vf4 v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) v[u] = ld16u<false>(xr + i + u * G * 4);   // stay in L2 for pass B
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            mm_acc(m, v[u].x);
                            mm_acc(m, v[u].y);
                            mm_acc(m, v[u].z);
                            mm_acc(m, v[u].w);
                        }
                    }
                    for (; i < inner4; i += G * 4) {
                        const vf4 v = ld16u<false>(xr + i);
                        mm_acc(m, v.x);
                        mm_acc(m, v.y);
                        mm_acc(m, v.z);
                        mm_acc(m, v.w);
                    }
                    for (int j = inner4 + sub; j < inner; j += G) mm_acc(m, xr[j]);
                }
                for (int off = G >> 1; off >= 1; off >>= 1) {
                    m.mn = fminf(m.mn, __shfl_xor(m.mn, off, 64));
                    m.mx = fmaxf(m.mx, __shfl_xor(m.mx, off, 64));
                    m.nan |= __shfl_xor(m.nan, off, 64);
                }
                if (r < R && sub == 0) {
                    if (m.nan) m.mn = m.mx = __builtin_nanf("");
                    if (MODE == kModeMinMax) {
                        fold_store(m.mn, m.mx, r0 + r, row_min, row_max, maxval_out, fa);
                    } else {
                        const float mv = fabsf(tmax(fabsf(m.mn), m.mx));   // fp8_quantizer.py:236
                        if (row_min) row_min[r0 + r] = m.mn;
                        if (row_max) row_max[r0 + r] = m.mx;
                        if (maxval_out) maxval_out[r0 + r] = mv;
                        rowmv[r] = mv;
                    }
                }
            }
            if (MODE == kModeMinMax) continue;
            __syncthreads();
        }
        {
            const float *mvsrc = MODE == kModeQuant ? maxval + r0 : rowmv;
            // thread j <-> row j: channel constants, then the row's whole {s, 1/s} table from registers
            for (int j = tid; j < R; j += BS) {
                const Chan c = make_chan_fast(mvsrc[j], f, ftab);
                chans[j] = c;
                if (LUT) lut_row(lut + j * a.lut_stride, c, f);
            }
            __syncthreads();
        }
        // ---- pass B: the R rows are one contiguous range -> flat, fully coalesced 16-byte I/O.
        // The channel of a 16-byte group comes from one magic division.  A group that straddles
        // a row boundary is completed from an LDS patch: one thread per boundary first quantizes
        // the <= 3 elements that follow it (with the next row's constants), so every store of the
        // body is a full aligned 16 bytes (no partial-line read-modify-write in HBM).
        {
            auto quant_at = [&](int i) -> float {
                const int ch = div_small((uint32_t)i, a.magic);
                if (LUT) return quant_one(xt[i], lite_lds(chans + ch), lut + ch * a.lut_stride, pmaxf, f.qthr);
                return quant_direct(xt[i], chans[ch], f.M);
            };
            for (int i = tid; i < head; i += BS) yt[i] = quant_at(i);
            for (int i = bend + tid; i < n; i += BS) yt[i] = quant_at(i);
            // patches: row c+1 starts at local index (c+1)*inner
            for (int c = tid; c < R - 1; c += BS) {
                const int idx = (c + 1) * inner;
                float pv[3] = {0.0f, 0.0f, 0.0f};
                if (idx > head && idx < bend) {
                    const int end = head + (((idx - head) + 3) & ~3);   // end of the straddling group
                    for (int i = idx, k = 0; i < end; ++i, ++k) pv[k] = quant_at(i);   // 0..3 elements
                }
                patch[c] = make_float4(pv[0], pv[1], pv[2], 0.0f);
            }
            __syncthreads();
            for (int j0 = tid; j0 < nvec; j0 += BS * U) {
                vf4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j0 + u * BS < nvec) v[u] = ld16u<NT>(xt + head + (j0 + u * BS) * 4);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = j0 + u * BS;
                    if (j >= nvec) break;
                    const int o = head + j * 4;
                    const int ch = div_small((uint32_t)o, a.magic);
                    const int b = inner - (o - ch * inner);        // elements left in this row (>= 1)
                    float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                    if (LUT) {
                        quant_group<4>(e, lite_lds(chans + ch), lut + ch * a.lut_stride, pmaxf, f.qthr);
                    } else {
                        const Chan c = chans[ch];
#pragma unroll
                        for (int q = 0; q < 4; ++q) e[q] = quant_direct(e[q], c, f.M);
                    }
                    if (b < 4) {   // e[b..3] belong to the next row: take them from its patch
                        const float4 pt = patch[ch];
                        e[3] = b == 3 ? pt.x : (b == 2 ? pt.y : pt.z);
                        if (b < 3) e[2] = b == 2 ? pt.x : pt.y;
                        if (b < 2) e[1] = pt.x;
                    }
                    st16u<NT>(yt + o, vf4{e[0], e[1], e[2], e[3]});
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Short rows, flat: k_rows_flat (MODE 0 = K1, MODE 1 = fused K2+K5+K1), x and y 16-byte aligned.
// HBM wants what a plain grid-stride copy does: every block moves one ALIGNED 16 KiB chunk per step
// and concurrently running blocks touch neighbouring chunks (copy-kernel sweep, docs/HISTORY.md: 6.3-6.4 TB/s;
// a block that owns 128 contiguous KiB, or row-aligned chunks of 16 464 B: 5.2-5.7).  So the tensor
// is cut by ADDRESS, not by rows: chunk c = elements [4096 c, 4096 (c+1)); a tile = nch chunks
// (t*nch + i) * gridDim + blockIdx, i < nch; rows are whatever overlaps a chunk (a row cut by a chunk
// border gets its table built by both neighbours).  Per tile:
//   geometry  one thread per chunk: first row, phase within it, rows overlapped   (1 64-bit division)
//   pass A    (MODE 1) min/max of every overlapping row, G lanes per row; the chunk in which a row
//             STARTS writes row_min / row_max / maxval_out
//   tables    thread <-> (chunk, row): channel constants + the {s, 1/s} table
//   patches   first elements of a row up to the next 16-byte boundary, quantized with THAT row's
//             constants (so the streaming loop only issues whole aligned 16-byte stores); tail scalars
//   stream    one chunk per step: 4 x 16 B in flight per lane, channel of a group by magic division
// LDS: ChunkInfo[8] | float4 patch[Rt] | float4 chanlite[Rt] | float2 lut[Rt * stride] | float rowmv[Rt]
// ---------------------------------------------------------------------------------------------
template <int MODE, bool NT>
__global__ void __launch_bounds__(kBlock, 4)
k_rows_flat(const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ maxval,
            float *row_min, float *row_max, float *maxval_out, QFmt f, FlatArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double ftab[kFastTabSize];
    const int Rt = a.rpc * a.nch;
    ChunkInfo *cinfo = reinterpret_cast<ChunkInfo *>(smem);
    float4 *patch = reinterpret_cast<float4 *>(cinfo + kFlatMaxCh);
    float4 *chl = patch + Rt;
    float2 *lut = reinterpret_cast<float2 *>(chl + Rt);
    float *rowmv = reinterpret_cast<float *>(lut + Rt * a.lut_stride);
    const int tid = threadIdx.x;
    const int inner = a.inner;
    const int64_t G = gridDim.x;
    const float pmaxf = (float)f.pmax;
    for (int i = tid; i < kFastTabSize; i += kBlock) ftab[i] = kFastTab[i];

    for (int64_t c0 = blockIdx.x; c0 < a.nchunks; c0 += G * a.nch) {
        int nct = 1;
        while (nct < a.nch && c0 + nct * G < a.nchunks) ++nct;
        const int nlr = nct * a.rpc;
        __syncthreads();   // the previous tile's tables are no longer read (and ftab is staged)
        if (tid < nct) {
            const int64_t c = c0 + tid * G;
            const int64_t elo = c * kChunkElems;
            const int64_t rem = a.nvec * 4 - elo;
            ChunkInfo ci;
            ci.len = rem < kChunkElems ? (int)rem : kChunkElems;
            ci.tail = (c == a.nchunks - 1) ? a.tail : 0;
            ci.row_lo = elo / inner;
            ci.phase = (int)(elo - ci.row_lo * inner);
            ci.nrows = (ci.phase + ci.len + ci.tail - 1) / inner + 1;
            ci.pad[0] = ci.pad[1] = 0;
            cinfo[tid] = ci;
        }
        __syncthreads();
        if (MODE == kModeFused) {
            const int Gl = a.group, rpp = kBlock / Gl, sub = tid & (Gl - 1), slot = tid / Gl;
            const int inner4 = inner & ~3;
            for (int lrb = 0; lrb < nlr; lrb += rpp) {
                const int lr = lrb + slot;
                const int i = div_small((uint32_t)lr, a.rmagic), r = lr - i * a.rpc;
                const bool valid = lr < nlr && r < cinfo[i].nrows;
                MinMax m;
                mm_init(m);
                if (valid) {
                    const float *xr = x + (cinfo[i].row_lo + r) * inner;   // rows start at any 4-byte phase
                    int j = sub * 4;
                    for (; j + 3 * Gl * 4 < inner4; j += Gl * 16) {
                        vf4 v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) v[u] = ld16u<false>(xr + j + u * Gl * 4);   // stay in L2 for pass B
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            mm_acc(m, v[u].x);
                            mm_acc(m, v[u].y);
                            mm_acc(m, v[u].z);
                            mm_acc(m, v[u].w);
                        }
                    }
                    for (; j < inner4; j += Gl * 4) {
                        const vf4 v = ld16u<false>(xr + j);
                        mm_acc(m, v.x);
                        mm_acc(m, v.y);
                        mm_acc(m, v.z);
                        mm_acc(m, v.w);
                    }
                    for (int k = inner4 + sub; k < inner; k += Gl) mm_acc(m, xr[k]);
                }
                for (int off = Gl >> 1; off >= 1; off >>= 1) {
                    m.mn = fminf(m.mn, __shfl_xor(m.mn, off, 64));
                    m.mx = fmaxf(m.mx, __shfl_xor(m.mx, off, 64));
                    m.nan |= __shfl_xor(m.nan, off, 64);
                }
                if (valid && sub == 0) {
                    if (m.nan) m.mn = m.mx = __builtin_nanf("");
                    const float mv = fabsf(tmax(fabsf(m.mn), m.mx));   // fp8_quantizer.py:236
                    rowmv[lr] = mv;
                    if (r > 0 || cinfo[i].phase == 0) {   // the row starts in this chunk: this block reports it
                        const int64_t grow = cinfo[i].row_lo + r;
                        if (row_min) row_min[grow] = m.mn;
                        if (row_max) row_max[grow] = m.mx;
                        if (maxval_out) maxval_out[grow] = mv;
                    }
                }
            }
            __syncthreads();
        }
        for (int lr = tid; lr < nlr; lr += kBlock) {
            const int i = div_small((uint32_t)lr, a.rmagic), r = lr - i * a.rpc;
            if (r < cinfo[i].nrows) {
                const float mv = MODE != kModeFused ? maxval[cinfo[i].row_lo + r] : rowmv[lr];
                const Chan c = make_chan_fast(mv, f, ftab);
                chl[lr] = make_float4(c.maxv, c.minv, c.bias, c.pthr);
                lut_row(lut + lr * a.lut_stride, c, f);
            }
        }
        __syncthreads();
        // storage codes (N3): `x` / `y` are the fp32 side, the other pointer is a byte array of codes
        const int Mi = (int)f.M, sign_shift = f.sign_bits == 1 ? a.n_bits - 1 : -1;
        const uint8_t *codes_in = reinterpret_cast<const uint8_t *>(x);    // kModeDecode
        uint8_t *codes_out = reinterpret_cast<uint8_t *>(y);               // kModeEncode
        if (MODE != kModeDecode) {
            for (int lr = tid; lr < nlr; lr += kBlock) {
                const int i = div_small((uint32_t)lr, a.rmagic), r = lr - i * a.rpc;
                const ChunkInfo ci = cinfo[i];
                float pv[3] = {0.0f, 0.0f, 0.0f};
                if (r + 1 < ci.nrows) {
                    const int idx = (r + 1) * inner - ci.phase;   // chunk-local index of row r+1's first element
                    if (idx < ci.len && (idx & 3)) {
                        const float *xc = x + (c0 + i * G) * kChunkElems;
                        const ChanLite cl = lite_of(chl[lr + 1]);
                        const float2 *lt = lut + (lr + 1) * a.lut_stride;
                        for (int k = 0; k < 4 - (idx & 3); ++k)
                            pv[k] = MODE == kModeEncode
                                        ? __uint_as_float(encode_one(xc[idx + k], cl, lt, pmaxf, f.qthr, Mi, sign_shift))
                                        : quant_one(xc[idx + k], cl, lt, pmaxf, f.qthr);
                    }
                }
                patch[lr] = make_float4(pv[0], pv[1], pv[2], 0.0f);
            }
        }
        if (tid < cinfo[nct - 1].tail) {   // the tensor's last <= 3 elements
            const ChunkInfo ci = cinfo[nct - 1];
            const int e = ci.len + tid;
            const int lr = (nct - 1) * a.rpc + div_small((uint32_t)(ci.phase + e), a.magic);
            const int64_t at = (c0 + (nct - 1) * G) * kChunkElems + e;
            if (MODE == kModeEncode)
                codes_out[at] = (uint8_t)encode_one(x[at], lite_of(chl[lr]), lut + lr * a.lut_stride, pmaxf, f.qthr, Mi, sign_shift);
            else if (MODE == kModeDecode)
                y[at] = decode_one(codes_in[at], lut + lr * a.lut_stride, Mi, sign_shift);
            else
                y[at] = quant_one(x[at], lite_of(chl[lr]), lut + lr * a.lut_stride, pmaxf, f.qthr);
        }
        __syncthreads();
        constexpr int U = 4;
        if (MODE == kModeEncode || MODE == kModeDecode) {
            for (int i = 0; i < nct; ++i) {
                const int phase = cinfo[i].phase, ng = cinfo[i].len >> 2;
                const int64_t base = (c0 + i * G) * kChunkElems;
                const int lr0 = i * a.rpc;
                if (MODE == kModeEncode) {
                    // a lane converts FOUR CONSECUTIVE groups (16 elements: 64 contiguous bytes in, the line's other
                    // quarters hit L1) so that their codes leave as ONE 16-byte store: with lane <-> group and a dword
                    // store per group the kernel ran at 2.5 TB/s of its 5 B/element -- store-instruction bound
                    const vf4 *xv = reinterpret_cast<const vf4 *>(x + base);
                    uint32_t *cw = reinterpret_cast<uint32_t *>(codes_out + base);
                    const bool wide = (reinterpret_cast<uintptr_t>(cw) & 15) == 0;
                    vf4 v[U];
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (4 * tid + u < ng) v[u] = ld16<false>(xv + 4 * tid + u);
                    uint32_t word[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int q = 4 * tid + u;
                        word[u] = 0u;
                        if (q >= ng) break;
                        const int o = phase + 4 * q;
                        const int lrow = div_small((uint32_t)o, a.magic);
                        const int b = inner - (o - lrow * inner);   // elements left in this row (>= 1)
                        const int lr = lr0 + lrow;
                        const ChanLite cl = lite_of(chl[lr]);
                        const float2 *lt = lut + lr * a.lut_stride;
                        const float in[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                        uint32_t wd = encode_group4(in, cl, lt, pmaxf, f.qthr, Mi, sign_shift);
                        if (b < 4) {   // elements b..3 belong to the next row: its head patch holds their codes
                            const float4 pt = patch[lr];
                            const uint32_t c3 = __float_as_uint(b == 3 ? pt.x : (b == 2 ? pt.y : pt.z));
                            wd = (wd & 0x00ffffffu) | (c3 << 24);
                            if (b < 3) wd = (wd & 0xff00ffffu) | (__float_as_uint(b == 2 ? pt.x : pt.y) << 16);
                            if (b < 2) wd = (wd & 0xffff00ffu) | (__float_as_uint(pt.x) << 8);
                        }
                        word[u] = wd;
                    }
                    if (wide && 4 * tid + 3 < ng) {
                        *reinterpret_cast<uint4 *>(cw + 4 * tid) = make_uint4(word[0], word[1], word[2], word[3]);
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (4 * tid + u < ng) cw[4 * tid + u] = word[u];
                    }
                } else {
                    const uint32_t *cw = reinterpret_cast<const uint32_t *>(codes_in + base);
                    vf4 *yv = reinterpret_cast<vf4 *>(y + base);
                    uint32_t w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (tid + u * kBlock < ng) w[u] = cw[tid + u * kBlock];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int q = tid + u * kBlock;
                        if (q >= ng) break;
                        const int o = phase + 4 * q;
                        const int lrow = div_small((uint32_t)o, a.magic);
                        const int b = inner - (o - lrow * inner);
                        const float2 *la = lut + (lr0 + lrow) * a.lut_stride, *lb = la + a.lut_stride;   // this row / the next
                        st16<NT>(yv + q, vf4{decode_one(w[u] & 255u, la, Mi, sign_shift),
                                             decode_one((w[u] >> 8) & 255u, b > 1 ? la : lb, Mi, sign_shift),
                                             decode_one((w[u] >> 16) & 255u, b > 2 ? la : lb, Mi, sign_shift),
                                             decode_one(w[u] >> 24, b > 3 ? la : lb, Mi, sign_shift)});
                    }
                }
            }
            continue;
        }
        for (int i = 0; i < nct; ++i) {
            const int phase = cinfo[i].phase, ng = cinfo[i].len >> 2;
            const int64_t base = (c0 + i * G) * kChunkElems;
            const vf4 *xv = reinterpret_cast<const vf4 *>(x + base);
            vf4 *yv = reinterpret_cast<vf4 *>(y + base);
            const int lr0 = i * a.rpc;
            vf4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (tid + u * kBlock < ng) v[u] = ld16<NT>(xv + tid + u * kBlock);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = tid + u * kBlock;
                if (q >= ng) break;
                const int o = phase + 4 * q;
                const int lrow = div_small((uint32_t)o, a.magic);
                const int b = inner - (o - lrow * inner);   // elements left in this row (>= 1)
                const int lr = lr0 + lrow;
                float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                quant_group<4>(e, lite_of(chl[lr]), lut + lr * a.lut_stride, pmaxf, f.qthr);
                if (b < 4) {   // e[b..3] belong to the next row: take them from its patch
                    const float4 pt = patch[lr];
                    e[3] = b == 3 ? pt.x : (b == 2 ? pt.y : pt.z);
                    if (b < 3) e[2] = b == 2 ? pt.x : pt.y;
                    if (b < 2) e[1] = pt.x;
                }
                st16<NT>(yv + q, vf4{e[0], e[1], e[2], e[3]});
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Short rows, fused, staged: k_rows_staged does what k_rows_flat<1> does but fetches every element ONCE.
// k_rows_flat<1> finds the row ranges with a first pass over global memory and streams the chunk a
// second time; with ~1000 tiles in flight that second read has left L2 (PMC: 1.86x the tensor fetched,
// profiles/r01_pmc_other_kernels.json).  Here a block loads its aligned 4096-element chunk once
// (16 B per lane, coalesced, nontemporal) and parks it in LDS together with the head of the first and
// the tail of the last overlapping row (<= 255 scalars each, the neighbouring chunks' data); the row
// min/max, the boundary patches and the quantize pass all read LDS.  The loop is software-pipelined:
// the next chunk's loads are issued right after the current chunk is parked, so they fly during the
// four barrier phases.
// LDS: float win[kStagePad | 4096 | kStagePad] | float4 patch[rpc] | float4 chanlite[rpc] |
//      float2 lut[rpc * stride]
// patch[r] = the first (4 - start % 4) % 4 elements of row r, quantized: what the 16-byte group shared with row r-1 stores
// ---------------------------------------------------------------------------------------------
constexpr int kStagePad = 256;                                  // >= kFlatFusedMaxInner - 1, multiple of 4
constexpr int kStageWin = kStagePad + kChunkElems + kStagePad;  // floats
constexpr size_t kStageMaxLds = 36 * 1024;                      // dynamic LDS per block: 4 blocks per CU with the 3 KiB of statics
constexpr int kStageGrid = 2048;                                // persistent blocks (FP8Q_STAGED_GRID)
static_assert(kStagePad >= kFlatFusedMaxInner - 1 && kStagePad % 4 == 0, "border rows must fit the pads");

__device__ __forceinline__ ChunkInfo stage_geometry(int64_t c, const FlatArgs &a)
{
    ChunkInfo ci;
    const int64_t elo = c * kChunkElems;
    const int64_t rem = a.nvec * 4 - elo;
    ci.len = rem < kChunkElems ? (int)rem : kChunkElems;
    ci.tail = (c == a.nchunks - 1) ? a.tail : 0;
    ci.row_lo = div_rows(elo, a.inner);
    ci.phase = (int)(elo - ci.row_lo * a.inner);
    ci.nrows = div_small((uint32_t)(ci.phase + ci.len + ci.tail - 1), a.magic) + 1;
    ci.pad[0] = ci.nrows * a.inner - ci.phase - ci.len;   // elements of the last row behind the body (tail scalars included)
    ci.pad[1] = 0;
    return ci;
}

// The same geometry advanced from chunk c to chunk c + G WITHOUT a 64-bit division: the division of stage_geometry()
// is ~200 instructions of software long division, and with one thread computing it per chunk, ahead of a barrier, it sat
// on every chunk's critical path.  phase + G * 4096 < 2^32 / inner (checked by the caller), so the 32-bit magic division
// is exact; every thread computes the (wave-uniform) result itself: no LDS hand-off, no single-thread section.
__device__ __forceinline__ ChunkInfo stage_geometry_next(const ChunkInfo &cur, int64_t cn, uint32_t adv, const FlatArgs &a)
{
    ChunkInfo ci;
    const int64_t elo = cn * kChunkElems;
    const int64_t rem = a.nvec * 4 - elo;
    ci.len = rem < kChunkElems ? (int)rem : kChunkElems;
    ci.tail = (cn == a.nchunks - 1) ? a.tail : 0;
    const uint32_t t = (uint32_t)cur.phase + adv;
    const uint32_t q = (uint32_t)div_small(t, a.magic);
    ci.row_lo = cur.row_lo + q;
    ci.phase = (int)(t - q * (uint32_t)a.inner);
    ci.nrows = div_small((uint32_t)(ci.phase + ci.len + ci.tail - 1), a.magic) + 1;
    ci.pad[0] = ci.nrows * a.inner - ci.phase - ci.len;
    ci.pad[1] = 0;
    return ci;
}

// ---- pieces shared by k_rows_staged and k_rows_staged_mm (one 4096-element chunk per step, 256 threads) --------------
constexpr int kStageU = 4;   // 16-byte groups per lane and chunk

// the chunk's aligned body: 4 x 16 B per lane, coalesced (needs only the chunk index)
template <bool NT>
__device__ __forceinline__ void stage_load_body(const float *x, int64_t c, const FlatArgs &a, vf4 (&v)[kStageU])
{
    const int64_t elo = c * kChunkElems;
    const int64_t rem = a.nvec * 4 - elo;
    const int ng = (rem < kChunkElems ? (int)rem : kChunkElems) >> 2;
    const vf4 *xv = reinterpret_cast<const vf4 *>(x + elo);
#pragma unroll
    for (int u = 0; u < kStageU; ++u)
        if ((int)threadIdx.x + u * kBlock < ng) v[u] = ld16<NT>(xv + threadIdx.x + u * kBlock);
}

// head of the first and tail of the last overlapping row: <= 255 scalars each, one per thread (needs the geometry)
__device__ __forceinline__ void stage_load_borders(const float *x, int64_t c, const ChunkInfo &ci, float &bh, float &bt)
{
    const int64_t elo = c * kChunkElems;
    const int tid = threadIdx.x;
    if (tid < ci.phase) bh = x[elo - ci.phase + tid];
    if (tid < ci.pad[0]) bt = x[elo + ci.len + tid];
}

// registers -> LDS window: body at [kStagePad, kStagePad + len), the border pieces right before / behind it
__device__ __forceinline__ void stage_park(float *win, const ChunkInfo &ci, const vf4 (&v)[kStageU], float bh, float bt)
{
    const int tid = threadIdx.x, ng = ci.len >> 2;
#pragma unroll
    for (int u = 0; u < kStageU; ++u)
        if (tid + u * kBlock < ng) *reinterpret_cast<vf4 *>(win + kStagePad + 4 * (tid + u * kBlock)) = v[u];
    if (tid < ci.phase) win[kStagePad - ci.phase + tid] = bh;
    if (tid < ci.pad[0]) win[kStagePad + ci.len + tid] = bt;
}

// min / max / NaN of row `wr[0, inner)` in the window over Gl = 2^gs (<= 8) adjacent lanes; every lane gets the result.
// Clamped indices re-read the last element: no remainder loop.  DPP butterflies: no LDS crossbar latency.
__device__ __forceinline__ MinMax stage_row_range(const float *wr, bool valid, int inner, int sub, int gs)
{
    const int Gl = 1 << gs, last = inner - 1;
    MinMax m;
    mm_init(m);
    if (valid) {
        for (int j = sub; j < inner; j += 4 * Gl) {
            const float t0 = wr[j], t1 = wr[min(j + Gl, last)], t2 = wr[min(j + 2 * Gl, last)], t3 = wr[min(j + 3 * Gl, last)];
            mm_acc(m, t0);
            mm_acc(m, t1);
            mm_acc(m, t2);
            mm_acc(m, t3);
        }
    }
    if (gs >= 1) mm_dpp<0xB1>(m);    // quad_perm [1,0,3,2]
    if (gs >= 2) mm_dpp<0x4E>(m);    // quad_perm [2,3,0,1]
    if (gs >= 3) mm_dpp<0x141>(m);   // row_half_mirror
    if (m.nan) m.mn = m.mx = __builtin_nanf("");
    return m;
}

template <bool NT>
__global__ void __launch_bounds__(kBlock, 4)
k_rows_staged(const float *__restrict__ x, float *__restrict__ y, float *row_min, float *row_max,
              float *maxval_out, QFmt f, FlatArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double ftab[kFastTabSize];
    float *win = reinterpret_cast<float *>(smem);
    float4 *patch = reinterpret_cast<float4 *>(win + kStageWin);
    float4 *chl = patch + a.rpc;
    float2 *lut = reinterpret_cast<float2 *>(chl + a.rpc);
    const int tid = threadIdx.x;
    const int inner = a.inner;
    const int64_t G = gridDim.x;
    const float pmaxf = (float)f.pmax;
    constexpr int U = kStageU;
    for (int i = tid; i < kFastTabSize; i += kBlock) ftab[i] = kFastTab[i];

    int64_t c = blockIdx.x;   // gridDim.x <= nchunks
    // chunk geometry lives in registers (wave-uniform), advanced incrementally: see stage_geometry_next()
    const uint32_t adv = (uint32_t)G * (uint32_t)kChunkElems;
    const bool inc_ok = (uint64_t)(G * kChunkElems + 256) * (uint64_t)inner < (1ull << 32);
    ChunkInfo cur = stage_geometry(c, a);
    vf4 v[U];
    float bh = 0.0f, bt = 0.0f;
    stage_load_body<NT>(x, c, a, v);   // prologue: the first chunk's loads
    stage_load_borders(x, c, cur, bh, bt);
    for (;;) {
        const int64_t elo = c * kChunkElems;
        const int phase = cur.phase, nrows = cur.nrows, len = cur.len;
        const int ng = len >> 2;
        stage_park(win, cur, v, bh, bt);
        const int64_t cn = c + G;
        const bool more = cn < a.nchunks;
        ChunkInfo nxt = cur;
        if (more) nxt = inc_ok ? stage_geometry_next(cur, cn, adv, a) : stage_geometry(cn, a);
        __syncthreads();
        if (more) {   // next chunk: in flight during the phases below
            stage_load_body<NT>(x, cn, a, v);
            stage_load_borders(x, cn, nxt, bh, bt);
        }
        {   // per row, Gl (<= 8) lanes: range from LDS -> channel constants -> table -> the row's head patch
            const int gs = a.group, Gl = 1 << gs, rpp = kBlock >> gs, sub = tid & (Gl - 1), rs = tid >> gs;
            const float *w0 = win + (kStagePad - phase);
            for (int rb = 0; rb < nrows; rb += rpp) {
                const int r = rb + rs;
                const bool valid = r < nrows;
                const MinMax m = stage_row_range(w0 + r * inner, valid, inner, sub, gs);   // in every lane of the row
                if (valid) {
                    const float mv = fabsf(tmax(fabsf(m.mn), m.mx));   // fp8_quantizer.py:236
                    if (sub == 0 && (r > 0 || phase == 0)) {   // the row starts in this chunk: this block reports it
                        const int64_t grow = cur.row_lo + r;
                        if (row_min) row_min[grow] = m.mn;
                        if (row_max) row_max[grow] = m.mx;
                        if (maxval_out) maxval_out[grow] = mv;
                    }
                    const Chan ch = make_chan_fast(mv, f, ftab);   // the same in all Gl lanes (lockstep: no extra issue slots)
                    if (sub == 0) chl[r] = make_float4(ch.maxv, ch.minv, ch.bias, ch.pthr);
                    lut_part(lut + r * a.lut_stride, ch, f, sub, Gl);
                }
                // the table was written by this wave's own lanes: DS operations of a wave complete in order
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (valid) {
                    const int idx = r * inner - phase;   // chunk-local index of the row's first element
                    if (idx > 0 && idx < len && (idx & 3)) {   // it shares a 16-byte group with the previous row
                        const ChanLite cl = lite_of(chl[r]);
                        for (int k = sub; k < 4 - (idx & 3); k += Gl)
                            reinterpret_cast<float *>(patch)[4 * r + k] =
                                quant_one(win[kStagePad + idx + k], cl, lut + r * a.lut_stride, pmaxf, f.qthr);
                    }
                }
            }
        }
        __syncthreads();
        if (tid < cur.tail) {   // the tensor's last <= 3 elements
            const int e = len + tid;
            const int r = div_small((uint32_t)(phase + e), a.magic);
            y[elo + e] = quant_one(win[kStagePad + e], lite_of(chl[r]), lut + r * a.lut_stride, pmaxf, f.qthr);
        }
        {
            vf4 *yv = reinterpret_cast<vf4 *>(y + elo);
            vf4 w[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (tid + u * kBlock < ng) w[u] = *reinterpret_cast<const vf4 *>(win + kStagePad + 4 * (tid + u * kBlock));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = tid + u * kBlock;
                if (q >= ng) break;
                const int o = phase + 4 * q;
                const int lrow = div_small((uint32_t)o, a.magic);
                const int b = inner - (o - lrow * inner);   // elements left in this row (>= 1)
                float e[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
                quant_group<4, false>(e, lite_of(chl[lrow]), lut + lrow * a.lut_stride, pmaxf, f.qthr);   // fused: NaN rows are all-exact
                if (b < 4) {   // e[b..3] belong to the next row: its head patch
                    const float4 pt = patch[lrow + 1];
                    e[3] = b == 3 ? pt.x : (b == 2 ? pt.y : pt.z);
                    if (b < 3) e[2] = b == 2 ? pt.x : pt.y;
                    if (b < 2) e[1] = pt.x;
                }
                st16<NT>(yv + q, vf4{e[0], e[1], e[2], e[3]});
            }
        }
        if (!more) break;
        __syncthreads();   // the window and the tables are rewritten by the next chunk
        c = cn;
        cur = nxt;
    }
}

// K2 twin of k_rows_staged: per-row min/max (+ fold into the running estimate) of rows <= 256 elements at any row
// length and phase.  Loads are the aligned, coalesced 16 KiB chunks of a plain copy (the row-tiled kernel reads
// row-aligned tiles: 5.2-5.4 TB/s); LDS only transposes them for the G-lanes-per-row reduction.  No tables: 18.4 KiB of
// LDS and < 64 VGPRs, 8 blocks per CU.
template <bool NT>
__global__ void __launch_bounds__(kBlock, 8)
k_rows_staged_mm(const float *__restrict__ x, float *row_min, float *row_max, float *maxval_out, FoldArgs fa, FlatArgs a)
{
    __shared__ __attribute__((aligned(16))) float win[kStageWin];
    const int tid = threadIdx.x;
    const int inner = a.inner;
    const int64_t G = gridDim.x;
    int64_t c = blockIdx.x;   // gridDim.x <= nchunks
    const uint32_t adv = (uint32_t)G * (uint32_t)kChunkElems;
    const bool inc_ok = (uint64_t)(G * kChunkElems + 256) * (uint64_t)inner < (1ull << 32);
    ChunkInfo cur = stage_geometry(c, a);   // registers, wave-uniform (no single-thread section, no LDS hand-off)
    vf4 v[kStageU];
    float bh = 0.0f, bt = 0.0f;
    stage_load_body<NT>(x, c, a, v);
    stage_load_borders(x, c, cur, bh, bt);
    for (;;) {
        const int phase = cur.phase, nrows = cur.nrows;
        stage_park(win, cur, v, bh, bt);
        const int64_t cn = c + G;
        const bool more = cn < a.nchunks;
        ChunkInfo nxt = cur;
        if (more) nxt = inc_ok ? stage_geometry_next(cur, cn, adv, a) : stage_geometry(cn, a);
        __syncthreads();
        if (more) {
            stage_load_body<NT>(x, cn, a, v);
            stage_load_borders(x, cn, nxt, bh, bt);
        }
        {
            const int gs = a.group, Gl = 1 << gs, rpp = kBlock >> gs, sub = tid & (Gl - 1), rs = tid >> gs;
            const float *w0 = win + (kStagePad - phase);
            const int64_t row_lo = cur.row_lo;
            for (int rb = 0; rb < nrows; rb += rpp) {
                const int r = rb + rs;
                const bool valid = r < nrows;
                const MinMax m = stage_row_range(w0 + r * inner, valid, inner, sub, gs);
                if (valid && sub == 0 && (r > 0 || phase == 0))   // the chunk in which a row starts reports it
                    fold_store(m.mn, m.mx, row_lo + r, row_min, row_max, maxval_out, fa);
            }
        }
        if (!more) break;
        __syncthreads();   // the window is rewritten by the next chunk
        c = cn;
        cur = nxt;
    }
}

// BASELINE config 2 at its literal size (conv1 [64, 3, 7, 7]: 37 KB) and every other weight tensor that small: the launch is
// all latency.  k_rows_direct makes two passes (row min/max from global, tables, then the rows again as one flat range) around
// two workgroup barriers and builds R tables per workgroup in one thread each: 8.5 us for a tensor whose launch floor is ~4.
// Here a WAVE owns a row for the whole kernel: the row sits in registers (EPL elements per lane), min / max by wave shuffles,
// the channel constants once per wave, the {s, 1/s} table by the wave's 64 lanes into its own slice of LDS, the quantized row
// straight from the registers -- one pass, no workgroup barrier.  Same per-element arithmetic (quant_one) and the same min / max
// semantics (mm_acc, NaN flag) as the other fused routes: bit-identical results.
template <int EPL>
__global__ void __launch_bounds__(kBlock)
k_small_rows_fused(const float *__restrict__ x, float *__restrict__ y, int64_t C, int inner, float *row_min, float *row_max,
                   float *maxval_out, QFmt f)
{
    __shared__ float2 lut[kBlock / 64][kLutMax];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    if (row >= C) return;                       // (no workgroup barrier below)
    const float *xr = x + row * inner;
    float *yr = y + row * inner;
    float v[EPL];
    MinMax m;
    mm_init(m);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int i = lane + 64 * e;
        v[e] = 0.0f;
        if (i < inner) {
            v[e] = xr[i];
            mm_acc(m, v[e]);
        }
    }
    mm_wave_reduce(m);
    if (m.nan) m.mn = m.mx = __builtin_nanf("");
    const float mv = fabsf(tmax(fabsf(m.mn), m.mx));   // fp8_quantizer.py:236
    if (lane == 0) {
        if (row_min) row_min[row] = m.mn;
        if (row_max) row_max[row] = m.mx;
        if (maxval_out) maxval_out[row] = mv;
    }
    const Chan cfull = make_chan(mv, f);
    lut_part(lut[wave], cfull, f, lane, 64);
    __builtin_amdgcn_wave_barrier();
    const ChanLite c = lite(cfull);
    const float pmaxf = (float)f.pmax;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int i = lane + 64 * e;
        if (i < inner) yr[i] = quant_one(v[e], c, lut[wave], pmaxf, f.qthr);
    }
}

constexpr int64_t kSmallFusedElems = 16384;    // tensors up to 64 KB ...
constexpr int kSmallFusedInner = 512;          // ... of rows up to 8 elements per lane

}  // namespace

// K1 / K2: rows up to this length take k_rows_direct, longer ones the 2-D row kernels (measured
// cross-over: [58254,4608] K1 6.3 TB/s with k_quant_rows vs 5.5 with k_rows_direct).  The fused
// K2+K5+K1 path uses k_rows_direct up to kDirectMaxInner (5.1 TB/s at 4608 vs 3.9 two-pass).
int64_t fp8q_direct_max_inner()
{
    static const int v = [] {
        const char *e = getenv("FP8Q_DIRECT_MAX_INNER");   // tuning knob for experiments
        const int n = e ? atoi(e) : 0;
        return n >= 4 && n <= kDirectMaxInner ? n : 2047;
    }();
    return v;
}

// Chunks per tile of k_rows_flat: as many as `lds_bytes` of tables hold, at most max_nch, and for small tensors more
// blocks rather than longer tiles.  0: not even one chunk's tables fit.
static int64_t flat_nch(const FlatArgs &a, int64_t per_row, int64_t lds_bytes, int64_t max_nch)
{
    int64_t nch = (lds_bytes - (int64_t)kFlatMaxCh * sizeof(ChunkInfo)) / (a.rpc * per_row);
    if (nch > max_nch) nch = max_nch;
    while (nch > 1 && cdiv(a.nchunks, nch) < 1024) --nch;
    return nch;
}

static size_t flat_shmem(const FlatArgs &a, int64_t per_row) { return (size_t)kFlatMaxCh * sizeof(ChunkInfo) + (size_t)a.rpc * a.nch * per_row; }

// Launch k_rows_flat if the problem fits it; returns kNotFlat when the caller must use k_rows_direct
// (pointers not 16-byte aligned, rows too short for per-row tables in LDS, in-place fused, ...).
static int launch_rows_flat(int mode, const float *x, float *y, int64_t C, int64_t inner, const float *maxval,
                            float *row_min, float *row_max, float *maxval_out, const QFmt &f, hipStream_t st,
                            fp8q_rows_route_info *rec)
{
    static const int flat_env = env_int("FP8Q_FLAT", 1);   // FP8Q_FLAT=0: round-1 row-tiled kernel everywhere (A/B)
    if (!flat_env || mode == kModeMinMax || inner < 4) return kNotFlat;
    if ((((uintptr_t)x | (uintptr_t)y) & 15) != 0) return kNotFlat;
    if (mode == kModeFused && (inner > kFlatFusedMaxInner || x == y)) return kNotFlat;
    FlatArgs a = flat_geometry(C, inner, f.pmax + 1);
    const int64_t per_row = flat_per_row(a.lut_stride, mode == kModeFused);
    static const int lds_kb_env = [] {
        const char *e = getenv("FP8Q_FLAT_LDS_KB");
        const int v = e ? atoi(e) : 0;
        return v >= 4 && v <= 120 ? v : 36;
    }();
    static const int nch_env = [] {
        const char *e = getenv("FP8Q_FLAT_NCH");
        const int v = e ? atoi(e) : 0;
        // default 4: measured on K1 (tools/mb_flat_nch.py, one box, rows of 147 / 288 / 576 / 1152 / 2047 elements):
        // 4 chunks per tile 5.69 / 5.86 / 5.88 / 5.84 / 5.76 TB/s, 8 chunks 5.66 / 5.66 / 5.75 / 5.74 / 5.66, 2 chunks
        // 5.22 / 5.90 / 5.92 / 5.91 / 5.63, 1 chunk 4.27 / 5.44 / 5.44 / 5.41 / 4.62
        return v >= 1 && v <= kFlatMaxCh ? v : 4;
    }();
    const int64_t nch = flat_nch(a, per_row, (int64_t)lds_kb_env * 1024, nch_env);
    if (nch < 1) return kNotFlat;
    const bool nt = C * inner * 4 >= kNtBytes;
    if (mode == kModeFused) {   // one fetch per element: k_rows_staged, if window + tables leave room for 4 blocks per CU
        static const int staged_env = env_int("FP8Q_STAGED", 1);   // FP8Q_STAGED=0: two-pass k_rows_flat<1> (A/B)
        static const int staged_grid = [] {   // persistent grid cap; 0 = one chunk per block
            const char *e = getenv("FP8Q_STAGED_GRID");
            const int v = e ? atoi(e) : -1;
            return v >= 0 ? v : kStageGrid;
        }();
        const size_t sh = (size_t)kStageWin * sizeof(float) + (size_t)a.rpc * per_row;
        if (staged_env && sh <= kStageMaxLds) {
            int gs = 0;
            while (gs < 6 && (2 << gs) * a.rpc <= kBlock) ++gs;
            a.group = gs;   // log2(lanes per row) here
            a.nch = 1;
            const int64_t blocks = staged_grid ? balanced_blocks(a.nchunks, staged_grid) : a.nchunks;
            const auto fill = [&](fp8q_rows_route_info &r) {
                r.kernel = FP8Q_ROWS_K_ROWS_STAGED;
                r.nontemporal = nt;
                r.group = 1 << gs;
                r.nch = 1;
                r.grid_x = blocks;
                r.grid_y = 1;
            };
            return rows_emit(rec, fill, [&] {
                dispatch<true, false>(nt, [&](auto NT) {
                    hipLaunchKernelGGL((k_rows_staged<NT()>), dim3((unsigned)blocks), dim3(kBlock), sh, st, x, y, row_min, row_max,
                                       maxval_out, f, a);
                });
            });
        }
    }
    a.nch = (int)nch;
    int G = 1;
    while (G < 64 && (int64_t)G * 24 < inner) G <<= 1;
    a.group = G;
    static const int grid_env = env_int("FP8Q_FLAT_GRID", 0, 0);
    // Tensors beyond the caches: one tile per block (a grid of tens of thousands of short blocks streams 5-10 % faster
    // than a persistent one).  Cache-sized tensors (K1, <= 16384 chunks = 64 MiB): one tile per block means 1..16 ROUNDS of
    // the 1024 resident blocks, and a fractional last round is lost time (2352 tiles = 2.3 rounds pay for 3) -- a
    // resident grid striding over the chunks hands every block the same number +- 1 instead: [2^17,147] 40.2 -> 35.1 us,
    // [2^18,147] 66.2 -> 61.2, [30000,1152] 58.7 -> 51.4, [100000,576] 87.0 -> 83.1; at 36864 chunks it already loses
    // on 576 / 1152-element rows (207 -> 216..241 us), on the headline (75264 chunks) 408 -> 437..477.
    int64_t blocks = cdiv(a.nchunks, a.nch);
    const int64_t grid_cap = grid_env ? grid_env : ((mode == kModeQuant && a.nchunks <= 16384) ? 1024 : 32768);
    if (blocks > grid_cap) blocks = grid_cap;
    const auto fill = [&](fp8q_rows_route_info &r) {
        r.kernel = FP8Q_ROWS_K_ROWS_FLAT;
        r.nontemporal = nt;
        r.group = G;
        r.nch = a.nch;
        r.grid_x = blocks;
        r.grid_y = 1;
    };
    return rows_emit(rec, fill, [&] {
        dispatch<kModeQuant, kModeFused>(mode, [&](auto MODE) {
            dispatch<true, false>(nt, [&](auto NT) {
                hipLaunchKernelGGL((k_rows_flat<MODE(), NT()>), dim3((unsigned)blocks), dim3(kBlock), flat_shmem(a, per_row), st, x, y,
                                   maxval, row_min, row_max, maxval_out, f, a);
            });
        });
    });
}

// Storage codes of per-channel tensors with short rows through k_rows_flat (aligned 16 KiB chunks of the fp32 side,
// per-row tables in LDS): the row-per-block codec kernel spends a 256-thread block, a double-precision constant
// evaluation and a 33-entry table on every 147-element filter.  kNotFlat when the shape does not fit.
// Used by fp8q_codec.hip (same library, not part of the C ABI).
// rec: record the route instead of launching (route_emit; what fp8q_codec_route asks).
__attribute__((visibility("hidden"))) int fp8q_codec_flat_launch(bool encode, const void *in, void *out, int64_t C,
                                                                 int64_t inner, const float *maxval, const QFmt &f,
                                                                 int n_bits, hipStream_t st, fp8q_codec_route_info *rec)
{
    const void *fp = encode ? in : (const void *)out;       // the fp32 side
    const void *cp = encode ? (const void *)out : in;       // the code side
    if (inner < 4 || inner > fp8q_direct_max_inner() || ((uintptr_t)fp & 15) != 0 || ((uintptr_t)cp & 3) != 0) return kNotFlat;
    FlatArgs a = flat_geometry(C, inner, f.pmax + 1);
    a.n_bits = n_bits;
    const int64_t per_row = flat_per_row(a.lut_stride);
    const int64_t nch = flat_nch(a, per_row, 36 * 1024, 4);   // as K1's tiles (launch_rows_flat)
    if (nch < 1) return kNotFlat;
    a.nch = (int)nch;
    a.group = 1;
    const int64_t tiles = cdiv(a.nchunks, nch);
    int64_t blocks = tiles;
    if (blocks > 32768) blocks = 32768;
    const bool nt = C * inner * 4 >= kNtBytes;
    const float *xf = (const float *)in;    // encode: fp32 in; decode: the codes, reinterpreted inside the kernel
    float *yf = (float *)out;               // decode: fp32 out; encode: the codes
    const auto fill = [&](fp8q_codec_route_info &r) {
        r.kernel = FP8Q_CODEC_K_ROWS_FLAT;
        r.nontemporal = nt;
        r.nch = a.nch;
        r.wide = encode && ((uintptr_t)cp & 15) == 0;   // (a chunk's codes start a multiple of 4096 bytes behind the base)
        r.grid_x = blocks;
        r.grid_y = 1;
        r.steps = cdiv(tiles, blocks);
    };
    return route_emit(rec, fill, [&] {
        dispatch<kModeEncode, kModeDecode>(encode ? kModeEncode : kModeDecode, [&](auto MODE) {
            dispatch<true, false>(nt, [&](auto NT) {
                hipLaunchKernelGGL((k_rows_flat<MODE(), NT()>), dim3((unsigned)blocks), dim3(kBlock), flat_shmem(a, per_row), st, xf, yf,
                                   maxval, nullptr, nullptr, nullptr, f, a);
            });
        });
    });
}

// k_rows_staged_mm for [C, inner]: rows of 4..256 elements, x 16-byte aligned; kNotFlat otherwise
int fp8q_launch_rows_staged_mm(const float *x, int64_t C, int64_t inner, float *row_min, float *row_max, float *maxval_out,
                          const FoldArgs &fa, hipStream_t st, fp8q_rows_route_info *rec)
{
    static const int staged_env = env_int("FP8Q_STAGED", 1);   // FP8Q_STAGED=0: row-tiled k_rows_direct<2> (A/B)
    if (!staged_env || inner < 4 || inner > kFlatFusedMaxInner || ((uintptr_t)x & 15) != 0) return kNotFlat;
    FlatArgs a = flat_geometry(C, inner, 0);   // no tables
    int gs = 0;
    while (gs < 3 && (2 << gs) * a.rpc <= kBlock) ++gs;
    a.group = gs;
    // persistent-grid cap; 0 = one chunk per block (measured best: no stores to wait for)
    static const int grid_env = env_int("FP8Q_STAGED_MM_GRID", 0, 0);
    const int64_t blocks = grid_env ? balanced_blocks(a.nchunks, grid_env) : a.nchunks;
    const bool nt = C * inner * 4 >= kNtBytes;
    const auto fill = [&](fp8q_rows_route_info &r) {
        r.kernel = FP8Q_ROWS_K_ROWS_STAGED_MM;
        r.nontemporal = nt;
        r.group = 1 << gs;
        r.nch = 1;
        r.grid_x = blocks;
        r.grid_y = 1;
    };
    return rows_emit(rec, fill, [&] {
        dispatch<true, false>(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_rows_staged_mm<NT()>), dim3((unsigned)blocks), dim3(kBlock), 0, st, x, row_min, row_max, maxval_out,
                               fa, a);
        });
    });
}

// Launch k_rows_direct for [C, inner], inner <= kDirectMaxInner (any 4-byte aligned pointers).
int fp8q_launch_rows_direct(int mode, const float *x, float *y, int64_t C, int64_t inner, const float *maxval,
                       float *row_min, float *row_max, float *maxval_out, const QFmt &f,
                       const FoldArgs &fa, hipStream_t st, fp8q_rows_route_info *rec)
{
    {
        const int rc = launch_rows_flat(mode, x, y, C, inner, maxval, row_min, row_max, maxval_out, f, st, rec);
        if (rc != kNotFlat) return rc;
    }
    TileArgs a = {};
    a.inner = (int)inner;
    a.lut_stride = f.pmax + 1;
    a.lmagic = magic_of(a.lut_stride);
    a.magic = magic_of((int)inner);
    const bool lut = mode != kModeMinMax && inner >= 2 * (int64_t)a.lut_stride;
    // lanes per row: ~16-32 elements (4-8 dwordx4) per lane, power of two <= 64
    int G = 1;
    while (G < 64 && (int64_t)G * 24 < inner) G <<= 1;
    static const int elems_env = [] {   // tuning knob for experiments
        const char *e = getenv("FP8Q_DIRECT_ELEMS");
        const int v = e ? atoi(e) : 0;
        return v >= 256 && v <= (1 << 20) ? v : kDirectElems;
    }();
    const int BSZ = kBlock;
    const int rpp = BSZ / G;
    int64_t R = (elems_env * BSZ / 256) / inner;
    static const int mm_passes_env = env_int("FP8Q_K2_PASSES", 2);
    if (mode == kModeMinMax) R = mm_passes_env * rpp;   // no tables: a few passes per iteration
    if (R < rpp) R = rpp;                         // at least one full pass
    if (R > 256) R = 256;                         // one make_chan pass
    // tables + the 3 KiB of staged log2/exp2 tables must fit in 40 KiB of LDS (4 blocks per CU)
    const int64_t per_row = (int64_t)sizeof(Chan) + 4 + 16 + (lut ? (int64_t)a.lut_stride * 8 : 0);
    static const int lds_kb_env = [] {   // tuning knob: LDS budget of the per-row tables
        const char *e = getenv("FP8Q_DIRECT_LDS_KB");
        const int v = e ? atoi(e) : 0;
        return v >= 4 && v <= 120 ? v : 36;
    }();
    const int64_t lds_cap = (int64_t)lds_kb_env * 1024;
    if (R * per_row > lds_cap) R = lds_cap / per_row;
    const int64_t want = cdiv(C, 1024);           // small tensors: spread over >= ~1024 blocks
    if (R > want) R = want;
    if (R >= 4) R &= ~(int64_t)3;                 // keeps tile starts 16-byte aligned for any inner
    if (R < 1) R = 1;
    a.rows = (int)R;
    a.group = G;
    a.coaligned = (y == nullptr) || ((((uintptr_t)x ^ (uintptr_t)y) & 15) == 0);
    const size_t shmem = (size_t)((R + 3) & ~(int64_t)3) * 4 + (size_t)R * 16 + (size_t)R * sizeof(Chan) +
                         (lut ? (size_t)R * a.lut_stride * sizeof(float2) : 0);
    int64_t blocks = cdiv(C, R);
    // K2: many short blocks (two passes of rows each) measured best: 5.4 TB/s against 4.9 with 4096 x 4 passes
    static const int mm_blocks_env = env_int("FP8Q_K2_BLOCKS", 65536);
    const int64_t bcap = mode == kModeMinMax ? mm_blocks_env : 2 * kTargetBlocks;
    if (blocks > bcap) blocks = balanced_blocks(blocks, bcap);
    const bool nt = C * inner * 4 >= kNtBytes;
    const dim3 g((unsigned)blocks), b(BSZ);
    auto launch = [&](auto MODE, auto LUT, auto NT) {
        hipLaunchKernelGGL((k_rows_direct<MODE(), LUT(), NT()>), g, b, shmem, st, x, y, C, maxval, row_min, row_max,
                           maxval_out, f, a, fa);
    };
    const auto fill = [&](fp8q_rows_route_info &r) {
        r.kernel = FP8Q_ROWS_K_ROWS_DIRECT;
        r.nontemporal = mode != kModeMinMax && nt;      // (min/max has one instance)
        r.lut = lut;
        r.group = G;
        r.rows_per_block = (int)R;
        r.grid_x = blocks;
        r.grid_y = 1;
    };
    return rows_emit(rec, fill, [&] {
        if (mode == kModeMinMax) {   // no tables, no stores: one instantiation
            launch(Const<kModeMinMax>{}, Const<false>{}, Const<false>{});
        } else {
            dispatch<kModeQuant, kModeFused>(mode, [&](auto MODE) {
                dispatch<true, false>(lut, [&](auto LUT) { dispatch<true, false>(nt, [&](auto NT) { launch(MODE, LUT, NT); }); });
            });
        }
    });
}

extern "C" {

int64_t fp8q_fused_max_inner(void) { return kDirectMaxInner; }

int fp8q_minmax_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, float *row_min,
                             float *row_max, float *maxval_out, float mbits, int n_bits,
                             int sign_bits, fp8q_stream_t stream)
{
    return fp8q_minmax_quantize_plan(x, y, C, inner, row_min, row_max, maxval_out, mbits, n_bits, sign_bits, (hipStream_t)stream,
                                     nullptr);
}

// fp8q_minmax_quantize_f32 itself; rec: record the route instead of launching (rows_emit, fp8q_rows.h)
int fp8q_minmax_quantize_plan(const float *x, float *y, int64_t C, int64_t inner, float *row_min, float *row_max,
                              float *maxval_out, float mbits, int n_bits, int sign_bits, hipStream_t st,
                              fp8q_rows_route_info *rec)
{
    if (C < 0 || inner < 0) return FP8Q_EINVAL;
    QFmt f;
    if (int rc = make_fmt(mbits, n_bits, sign_bits, &f)) return rc;
    if (C == 0 || inner == 0) return FP8Q_OK;
    if (!x || !y) return FP8Q_EINVAL;
    if (inner > kDirectMaxInner) return FP8Q_ETOOLONG;
    if (((uintptr_t)x & 3) != 0 || ((uintptr_t)y & 3) != 0) return FP8Q_EINVAL;
    static const bool small_fused = env_int("FP8Q_SMALL_FUSED", 1) != 0;   // =0: the general routes for small tensors too (A/B)
    const FoldArgs nofold = {0, 1, 0.0f, 0.0f};
    if (small_fused && C * inner <= kSmallFusedElems && inner <= kSmallFusedInner) {
        int epl = 0;
        dispatch<1, 2, 3, 4, 8>((int)cdiv(inner, 64), [&](auto EPL) { epl = EPL(); });   // elements per lane: 5..8 take 8
        const auto fill = [&](fp8q_rows_route_info &r) {
            r.kernel = FP8Q_ROWS_K_SMALL_ROWS_FUSED;
            r.lanes = 64;
            r.slots = epl;
            r.grid_x = cdiv(C, kBlock / 64);
            r.grid_y = 1;
        };
        return rows_emit(rec, fill, [&] {
            dispatch<1, 2, 3, 4, 8>(epl, [&](auto EPL) {
                hipLaunchKernelGGL(k_small_rows_fused<EPL()>, dim3((unsigned)cdiv(C, kBlock / 64)), dim3(kBlock), 0, st, x, y, C,
                                   (int)inner, row_min, row_max, maxval_out, f);
            });
        });
    }
    const int rc = fp8q_launch_rows_reg(true, x, y, C, inner, row_min, row_max, maxval_out, f, nofold, st, rec);
    if (rc != kNotFlat) return rc;
    return fp8q_launch_rows_direct(kModeFused, x, y, C, inner, nullptr, row_min, row_max, maxval_out, f, nofold, st, rec);
}

}  // extern "C"
