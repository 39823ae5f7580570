/*
 * fp8q.h -- C ABI of the MI355X-native FP8 fake-quantization engine (libfp8q_hip.so).
 *
 * The reference (Qualcomm-AI-research/FP8-quantization) has no FFI: its "device boundary"
 * is the set of eager ATen op chains listed in SURVEY.md section 2.1.  Each entry point
 * below replaces one of those chains with one (or two) hand-written gfx950 kernels; the
 * Python classes that keep the reference's operator API (fp8-quantization_amd/quantization)
 * call them through ctypes with tensor.data_ptr() and the current HIP stream.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated or freed here
 *   - tensors are contiguous fp32, viewed as [C, inner] (per-channel = dim 0, as the
 *     reference does with x.view(x.shape[0], -1)); per-tensor calls pass C == 1
 *   - enqueue-only on `stream` (a hipStream_t, NULL = default stream); no host sync
 *   - return 0 on success, a positive hipError_t on a HIP failure, a negative FP8Q_E* on a
 *     bad argument; never throws; stateless and thread-safe
 *   - arithmetic contract: bit-identical to oracle/fp8q_oracle.c (reference op order in
 *     fp32, correctly rounded log2 / 2^x) -- see DESIGN.md "Arithmetic contract".  ONE exception:
 *     fp8q_mse_grid_f32 (K4) -- see its comment
 */
#ifndef FP8Q_H
#define FP8Q_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FP8Q_VERSION 601 /* 0.6.1: 0.6.0 (one-call MSE calibration step fp8q_mse_calibrate_f32, fused small-tensor routes) + sign_bits decided on the device (fp8q_sign_fold_u8, fp8q_quantize_ds_f32) */

#define FP8Q_OK 0
#define FP8Q_EINVAL (-1)       /* null pointer, negative size, n_maxval not in {1, C}, ... */
#define FP8Q_EUNSUPPORTED (-2) /* n_bits - sign_bits - M > 7 (more than 7 exponent bits) */
#define FP8Q_EWORKSPACE (-3)   /* workspace too small or misaligned */
#define FP8Q_ETOOLONG (-4)     /* fused min/max+quantize: rows longer than fp8q_fused_max_inner() */
#define FP8Q_ETOOMANY (-5)     /* MSE grid search: more than 65535 channels in one call */
#define FP8Q_ETIMEDOUT (-6)    /* fp8q_minmax_workspace_check: a min/max reducer gave up waiting (that range is NaN) */

/* range-estimator fold modes (how a new batch estimate is merged into the running one) */
#define FP8Q_FOLD_CURRENT 0 /* overwrite          range_estimators.py:72-73  CurrentMinMaxEstimator */
#define FP8Q_FOLD_ALL 1     /* min / max          range_estimators.py:97-98  AllMinMaxEstimator     */
#define FP8Q_FOLD_RUNNING 2 /* EMA (1-m)*new+m*cur range_estimators.py:122-123 RunningMinMaxEstimator */

/*
 * Workspaces of the min/max entry points (fp8q_minmax_f32, fp8q_affine_act_minmax_f32).  The two-stage reduction
 * runs in ONE launch: streaming blocks publish tagged partial results in the workspace, a reducer block collects them
 * and clears them again.  Contract: the workspace is ZERO before the first call that uses it (hipMemset once after
 * allocating it) and every call leaves it zero, so a buffer that is only ever handed to these two entry points, by one
 * stream at a time, never needs clearing again.  Do not share one buffer between launches that may run concurrently,
 * and do not let other kernels scribble over it.
 * Layout: a 16-byte header {uint32 timeout count, 12 reserved bytes} followed by the 8-byte granules.
 *
 * Failure modes and how they surface (the entry points only enqueue, so they cannot report what happens on the device):
 *   - the reducer block waits a bounded time (~2 s) for its streaming blocks; if one never arrives it writes NaN as
 *     that row's range AND increments the header's timeout count.  fp8q_minmax_workspace_check() -- which synchronises
 *     the stream -- then returns FP8Q_ETIMEDOUT; call it wherever a sync is acceptable (the Python layer does at
 *     fix_ranges(), i.e. once after calibration).
 *   - a workspace that was not zero on entry, or that two streams used at once, gives wrong ranges silently;
 *     fp8q_minmax_workspace_check() returns FP8Q_EWORKSPACE when it finds non-zero granules between calls, and with
 *     FP8Q_DEBUG_WS=1 in the environment every min/max call runs that check (sync + copy) on entry and refuses to
 *     launch on a dirty workspace.
 * Progress does not rely on the order in which workgroups are dispatched (streaming blocks never wait; reducers are at
 * most half of the resident workgroup slots); in-order dispatch -- what the hardware does, not a HIP guarantee -- only
 * keeps the reducer's wait short.
 */

typedef void *fp8q_stream_t; /* hipStream_t */

int fp8q_version(void);
const char *fp8q_strerror(int code);

/*
 * K1 -- FP8 quantize + dequantize.
 * Replaces quantize_to_fp8_ste_MM(x_float, n_bits, maxval, num_mantissa_bits, sign_bits),
 * quantization/quantizers/fp8_quantizer.py:91-133 (13 eager ATen kernels -> 1 launch).
 *   x, y     [C, inner] fp32 (y may alias x)
 *   maxval   [n_maxval] fp32, n_maxval == 1 (per tensor) or == C (per channel)
 *   mbits    number of mantissa bits; rounded half-to-even and clamped to [1, n_bits - sign_bits]
 *   sign_bits 1 (clamp to [-maxval, maxval]) or 0 (clamp to [0, maxval])
 * HBM traffic: 8 B / element.
 */
int fp8q_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval,
                      int64_t n_maxval, float mbits, int n_bits, int sign_bits,
                      fp8q_stream_t stream);

/*
 * K2/K3/K5 -- min/max range estimation with the running-estimate fold.
 * Replaces {Current,All,Running}MinMaxEstimator.forward, quantization/range_estimators.py:61-125
 * (x.min(), x.max(), torch.min/max fold) and the abs-max of FPQuantizer.set_quant_range,
 * fp8_quantizer.py:236.
 *   x         [C, inner] fp32 (C == 1: per tensor)
 *   cur_min, cur_max [C] running estimate, updated in place;  `first` != 0: no previous estimate
 *   maxval_out [C] or NULL: |max(|cur_min|, cur_max)| after the fold
 *   ws        8-byte aligned scratch of at least fp8q_minmax_workspace_bytes(C, inner) bytes, zero on first use (see above)
 * NaN anywhere in a row makes that row's min and max NaN (torch semantics).
 * Signed zeros: a zero minimum is -0.0 when the row holds a -0.0, a zero maximum is +0.0 when it holds a +0.0 (IEEE 754-2019
 * minimum / maximum, order-independent; ATen returns whichever zero its reduction met first, so the reference does not pin it).
 * HBM traffic: 4 B / element.
 */
size_t fp8q_minmax_workspace_bytes(int64_t C, int64_t inner);
int fp8q_minmax_f32(const float *x, int64_t C, int64_t inner, float *cur_min, float *cur_max,
                    float *maxval_out, int fold_mode, double momentum, int first, void *ws,
                    size_t ws_bytes, fp8q_stream_t stream);

/*
 * K2+K5+K1 fused -- per-channel weight quantization in estimate_ranges state:
 * QuantizationManager.forward (quantization_manager.py:114-122) with CurrentMinMaxEstimator
 * and set_maxval=True: row min/max -> maxval = |max(|min|, max)| -> quantize, rows staged in LDS.
 *   x, y [C, inner]; row_min,row_max,maxval_out [C] outputs (each may be NULL)
 * Requires inner <= fp8q_fused_max_inner(); larger rows: call fp8q_minmax_f32 + fp8q_quantize_f32.
 * HBM traffic: 8 B / element.
 */
/*
 * Batch-sharded (data-parallel) calibration: the _packed variants additionally write, per row, the 16-byte record
 * {-min, max, isnan(min), isnan(max)} of the FOLDED estimate ([C, 4] fp32, 16-byte aligned; a NaN travels as its
 * flag with -inf as the value).  The ranks then need ONE all-reduce(MAX) over that buffer -- min/max commute with the
 * union of the shards -- and fp8q_ranges_unpack_f32 turns the reduced records back into cur_min / cur_max (+ K5
 * maxval_out; each may be NULL).  The reference is single-process (utils/qat_utils.py:27-28); this is north_star's
 * "activation calibration is batch-sharded with an RCCL all-reduce of the running min/max" with no tensor glue
 * around the collective.
 */
int fp8q_minmax_packed_f32(const float *x, int64_t C, int64_t inner, float *cur_min, float *cur_max,
                           float *maxval_out, float *packed, int fold_mode, double momentum, int first, void *ws,
                           size_t ws_bytes, fp8q_stream_t stream);
int fp8q_ranges_unpack_f32(const float *packed, int64_t n, float *cur_min, float *cur_max, float *maxval_out,
                           fp8q_stream_t stream);

/*
 * SYNCHRONISES `stream`, then inspects a min/max workspace: FP8Q_ETIMEDOUT if a reducer timed out since the last
 * clear, FP8Q_EWORKSPACE if granules are non-zero between calls (contract violated), FP8Q_OK otherwise.
 * clear != 0: the workspace is zeroed again after a failure was reported (so the buffer stays usable).
 */
int fp8q_minmax_workspace_check(void *ws, size_t ws_bytes, int clear, fp8q_stream_t stream);

int64_t fp8q_fused_max_inner(void);
int fp8q_minmax_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, float *row_min,
                             float *row_max, float *maxval_out, float mbits, int n_bits,
                             int sign_bits, fp8q_stream_t stream);

/*
 * Which kernel of the row family the three entries above launch: fp8q_quantize_f32 (FP8Q_ROWS_QUANTIZE), fp8q_minmax_f32 with
 * its packed / linspace variants (FP8Q_ROWS_MINMAX) and fp8q_minmax_quantize_f32 (FP8Q_ROWS_MINMAX_QUANTIZE), for a [C, inner]
 * tensor of a format, at the process's settings (the FP8Q_* tuning variables as the launchers read them).  Host arithmetic
 * only: no launch, no device -- the entries' own code behind their argument checks, every launcher's geometry block and
 * dispatch included, with a callback that records instead of launching, so that a test can assert the route before it trusts a
 * shape.  per_channel: one range per row (n_maxval == C), else one for the tensor (the entries then see one row of C * inner
 * elements; the fused entry is per channel always).  x_mod16 / y_mod16: the addresses of x and y modulo 16 (y is ignored for
 * min/max); in_place: y == x (then y_mod16 must equal x_mod16).
 *   kernel          FP8Q_ROWS_K_* below; -1 with launches == 0 for an empty tensor
 *   nontemporal     the instance for tensors of 64 MiB and more (k_quant_scalar and the min/max k_rows_direct have one instance)
 *   small           k_quant_rows: the U = 1 pieces (4 KiB per block) of a cache-sized per-tensor row
 *   lut             k_rows_direct: per-row {s, 1/s} tables in LDS (rows of at least 2 * (pmax + 1) elements), else the exact scale
 *   lanes, slots    k_rows_reg: lanes per row (16, 32, 64, 256) and 16-byte groups per lane (2..8); k_small_rows_fused: 64
 *                   lanes and the elements per lane of its instance (1, 2, 3, 4, 8)
 *   group           lanes per row of k_rows_flat's first pass and of k_rows_direct (1..64), of k_rows_staged and of
 *                   k_rows_staged_mm (1..8 both: a chunk overlaps at least 18 rows of the at most 256 elements they take)
 *   nch             chunks of 4096 elements per tile: k_rows_flat 1..4, the staged kernels 1
 *   rows_per_block  k_rows_direct: R, the rows of one tile
 *   nsplit          k_minmax_partial: streaming blocks per row (grid_x has the reducer block on top when nsplit > 1)
 *   grid_x, grid_y  of the first launch
 *   launches        one per slab of 65535 rows (k_quant_rows / k_quant_scalar / k_minmax_partial), 1 elsewhere
 * Fields that do not apply to the kernel are 0.  Errors as the entry reports them for the shape: FP8Q_EINVAL (a negative size,
 * an address that is not a multiple of 4 in the fused entry, C * inner == 0 for min/max, op or a phase out of range, info
 * NULL), FP8Q_EUNSUPPORTED (the format), FP8Q_ETOOLONG (fused rows beyond fp8q_fused_max_inner()); `info` is written on
 * FP8Q_OK only.
 */
#define FP8Q_ROWS_QUANTIZE 0
#define FP8Q_ROWS_MINMAX 1
#define FP8Q_ROWS_MINMAX_QUANTIZE 2
#define FP8Q_ROWS_K_QUANT_ROWS 0       /* k_quant_rows: one row per blockIdx.y, 16-byte groups */
#define FP8Q_ROWS_K_QUANT_SCALAR 1     /* k_quant_scalar: x and y not 16-byte co-aligned */
#define FP8Q_ROWS_K_ROWS_FLAT 2        /* k_rows_flat: aligned 4096-element chunks, per-row tables in LDS; K1 or fused two-pass */
#define FP8Q_ROWS_K_ROWS_DIRECT 3      /* k_rows_direct: row tiles; K1, fused or min/max */
#define FP8Q_ROWS_K_ROWS_REG 4         /* k_rows_reg: the row in registers; fused or min/max */
#define FP8Q_ROWS_K_ROWS_STAGED 5      /* k_rows_staged: fused, the chunk parked in LDS */
#define FP8Q_ROWS_K_ROWS_STAGED_MM 6   /* k_rows_staged_mm: its min/max twin */
#define FP8Q_ROWS_K_SMALL_ROWS_FUSED 7 /* k_small_rows_fused: a wave per row, tensors up to 16384 elements */
#define FP8Q_ROWS_K_MINMAX_PARTIAL 8   /* k_minmax_partial: long rows, per tensor */
typedef struct fp8q_rows_route_info {
    int kernel;
    int nontemporal;
    int small;
    int lut;
    int lanes, slots;
    int group;
    int nch;
    int rows_per_block;
    int nsplit;
    int launches;
    int reserved;
    int64_t grid_x, grid_y;
} fp8q_rows_route_info;
int fp8q_rows_route(int op, int64_t C, int64_t inner, int per_channel, float mbits, int n_bits, int sign_bits, int x_mod16,
                    int y_mod16, int in_place, fp8q_rows_route_info *info);

/*
 * K4 -- FP-MSE grid search accumulation.
 * Replaces the double loop of FP_MSE_Estimator.forward, quantization/range_estimators.py:337-347
 * (111 * |mbits| full quantizer passes -> one pass over x).
 *   x     [C, inner];  grid [n_cand, C] candidate maxvals;  mbits [n_m] (host array)
 *   mses  [n_m, n_cand, C] fp32, accumulated:  += mean over the row of (x - q(x))^2
 *   ws    scratch of at least fp8q_mse_workspace_bytes(C, inner, n_cand, n_m) bytes
 * Table entries agree with the oracle's to ~1e-7 relative (tests and tests/soak.py: <= 1e-5 on EVERY entry; the CHOSEN
 * (mantissa bits, maxval) equal to the oracle's choice or its oracle-MSE within 1e-6 relative of the oracle's minimum --
 * SURVEY.md 8c).  Every element takes the grid point the reference gives it; what differs is the summation: fp32 squares
 * summed in another order (double partials) or, on the interval-histogram route, exact sums.  Three routes, chosen by the
 * SHAPE of the call only (a tensor is evaluated the same way every time):
 *   rows < 2048 elements      lane = candidate, x broadcast from LDS: x * 2^frac(bias) scaled by the binade's power of two and
 *                             rounded with v_rndne; elements within 5 ulps of a rounding tie (the product carries up to 4 ulps
 *                             of error against the reference's fl32(x / s)) take the reference's own division;
 *   longer rows               lane = element, candidates walked with wave-uniform constants: the same product rounded on its
 *                             bits / by a magic-number add; every lane watches how close its elements come to a tie and the
 *                             elements within 5 ulps are re-evaluated with the reference's division (round 5: before, such an
 *                             element could take the other neighbour, which moved entries carried by a few elements -- the
 *                             search grid's last candidate 1.2 max|x| puts the largest element on a tie for M = 1, 3, 5 -- by up
 *                             to 4e-5);
 *   per-tensor rows (C == 1) of >= 16384 and < 2^31 elements, formats of <= 8 bits (all widths signed or all unsigned), at most
 *   4096 (width, candidate) pairs: FP_MSE_Estimator with or without the mantissa search, LineSearchEstimator's 1000
 *   candidates                the interval histogram (csrc/fp8q_mse_hist.hip): a quantizer is a step function of |x|, so the
 *                             exact borders of all cells of all candidates (the smallest float at which the reference's own
 *                             fp32 decisions flip) cut |x| into intervals; the nonzero keys are partitioned ONCE by their top
 *                             11 bits, integer moments {n, sum d, sum d^2} of every interval are accumulated with LDS atomics
 *                             (exact, order-independent: the result is deterministic), and a candidate's cells are summed as
 *                             S2 - 2 q S1 + n q^2 in double-double (the terms cancel to 1e-13 of S2 on already-quantized
 *                             data).  Cost independent of the number of candidates: ~4 ps per element.
 * fp8q_mse_workspace_bytes() accounts for the partitioned keys (4 B / element) and the border tables when the shape can take
 * the third route.  FP8Q_MSE_HIST=0 keeps the lane-per-element kernel; =2 evaluates every candidate of that route element
 * by element (the tests' cross-check of the cell logic).
 */
size_t fp8q_mse_workspace_bytes(int64_t C, int64_t inner, int64_t n_cand, int n_m);
int fp8q_mse_grid_f32(const float *x, int64_t C, int64_t inner, const float *grid, int64_t n_cand,
                      const float *mbits_host, int n_m, int n_bits, int sign_bits, float *mses,
                      void *ws, size_t ws_bytes, fp8q_stream_t stream);

/*
 * Which of K4's routes a call takes, and the size-dependent choices inside it: what fp8q_mse_grid_f32 (and the table step of
 * fp8q_mse_calibrate_f32) would launch for this shape and these formats with a 4-byte-aligned x.  Host arithmetic only -- no
 * launch, no device access, no allocation -- computed by the functions the launcher itself calls, so that a test can assert
 * the kernel its shape reaches and a moved threshold fails that test instead of emptying it.  Arguments are checked as
 * fp8q_mse_grid_f32 checks them (FP8Q_EINVAL, FP8Q_ETOOMANY, FP8Q_EUNSUPPORTED); `out` is written on FP8Q_OK only.
 */
typedef struct fp8q_mse_route_info {
    int kernel;               /* 0 k_mse_grid (lane = candidate), 1 k_mse_row (lane = element), 2 the interval histogram */
    int finish;               /* the launch that turns partial sums into table entries: 0 none (the kernel writes the table
                                 itself), 1 k_mse_final_tile (<= 32 partial sums per row), 2 k_mse_final */
    int64_t nsplit;           /* partial sums per (channel, width, candidate) row; 0 on the histogram route */
    /* histogram route only (0 elsewhere) */
    int tiles_per_wg;         /* 8192-key tiles per partition workgroup */
    int part_wgs;             /* partition workgroups (<= 768) */
    int slice_min;            /* smallest key slice of a k_moments unit: 2048 ... 16384 */
    int moments_threads;      /* threads per k_moments workgroup: 512 or 256 */
    int64_t n_superblocks;    /* 1024-interval superblocks of the prefix scan */
    int top_scan;             /* 1: more than 512 superblocks, k_iv_scan_top runs between the scan and the evaluation */
    int reserved;
} fp8q_mse_route_info;
int fp8q_mse_route(int64_t C, int64_t inner, int64_t n_cand, const float *mbits_host, int n_m, int n_bits, int sign_bits,
                   fp8q_mse_route_info *out);

/*
 * Sync-free MSE calibration.  The reference's FP_MSE_Estimator goes back to the host three times per call
 * (range_estimators.py:305 mx.item() for the search grid, :353 torch.mode(...).item() for the mantissa vote, :360 one
 * gather per channel); these entry points keep all of it on the device:
 *   fp8q_mse_linspace_f32  grid[i, c] = torch.linspace(lo_frac * mx[c], hi_frac * mx[c], n_cand)[i], bit for bit
 *                          ([n_cand, C]; the reference uses 0.1, 1.2 and 111: :296-305)
 *   fp8q_mse_select_f32    :350-369 on mses [n_m, n_cand, C] / grid [n_cand, C]: per channel the width with the smallest
 *                          minimum, the plurality vote over the channels (torch.mode: smallest value on a tie) ->
 *                          mbits_out[0] = mbits_host[vote] (DEVICE scalar), vote_out[0] = its index (may be NULL), per
 *                          channel maxval_out[c] = grid[argmin_i mses[vote, i, c], c] and xmin_out[c] = -sign_bits *
 *                          maxval (may be NULL).  torch.min / argmin semantics: first index of the minimum, NaN first.
 *                          ONE launch (round 5).  ws: at least fp8q_mse_select_workspace_bytes(C, n_m) bytes, 4-byte
 *                          aligned; its first 4096 bytes (the ticket block) follow the min/max workspace contract: zero
 *                          before the first call that uses the buffer, zero again after every call (counters by which the
 *                          last workgroup of a launch finds out that it is the last; fp8q_mse_calibrate_f32 uses the same
 *                          block for the per-tensor selection it appends to the table-finishing launch).
 *   fp8q_quantize_dm_f32   K1 (fp8q_quantize_f32) with the mantissa width read from a DEVICE scalar, so that the batch
 *                          that follows the vote in the same calibration forward needs no host round trip.  One row
 *                          per workgroup column whatever the row length: a calibration path, not the tuned K1 routes.
 */
int fp8q_mse_linspace_f32(const float *mx, int64_t C, int n_cand, double lo_frac, double hi_frac, float *grid,
                          fp8q_stream_t stream);
/* The first calibration batch of FP_MSE_Estimator in one launch: the row min / max (fp8q_minmax_f32, current fold), K5's
 * maxval_out[c] = |max(|min|, max)| = max|x| of the row, and the search grid of that maximum (what fp8q_mse_linspace_f32
 * would make of maxval_out), written by the thread that stores the row's range.  grid [n_cand, C]; workspace as fp8q_minmax_f32.
 * C <= 65535 (FP8Q_ETOOMANY, as fp8q_mse_grid_f32). */
int fp8q_minmax_linspace_f32(const float *x, int64_t C, int64_t inner, float *cur_min, float *cur_max, float *maxval_out,
                             float *grid, int n_cand, double lo_frac, double hi_frac, void *ws, size_t ws_bytes,
                             fp8q_stream_t stream);
size_t fp8q_mse_select_workspace_bytes(int64_t C, int n_m);
int fp8q_mse_select_f32(const float *mses, const float *grid, int64_t C, int64_t n_cand, const float *mbits_host, int n_m,
                        int sign_bits, float *mbits_out, int *vote_out, float *maxval_out, float *xmin_out, void *ws,
                        size_t ws_bytes, fp8q_stream_t stream);
int fp8q_quantize_dm_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                         const float *mbits_dev, int n_bits, int sign_bits, fp8q_stream_t stream);

/*
 * FPQuantizer with allow_unsigned=True (quantization/quantizers/fp8_quantizer.py:216-225): set_quant_range() switches the
 * quantizer to an unsigned format (sign_bits = 0, for good) when every range minimum is >= 0 -- in the reference a host
 * round trip per call (`torch.all(x_min >= 0)` inside an `if`).  Here the decision stays on the device:
 *   fp8q_sign_fold_u8      signed_flag[0] (1 = signed; the caller initialises it to 1) is cleared when all C values of x_min
 *                          are >= 0 (a NaN minimum keeps the sign bit, as the reference's comparison does); never set again.
 *   fp8q_quantize_ds_f32   K1 (fp8q_quantize_f32) with sign_bits read from that flag: both formats of the width travel by
 *                          value, every workgroup picks one.  Same launch geometry as fp8q_quantize_dm_f32.
 *   fp8q_quantize_dms_f32  the same with the width read from device memory as well.
 */
int fp8q_sign_fold_u8(const float *x_min, int64_t C, unsigned char *signed_flag, fp8q_stream_t stream);
int fp8q_quantize_ds_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                         float mbits, int n_bits, const unsigned char *signed_flag, fp8q_stream_t stream);
/* ... with the mantissa width in device memory too (fp8q_quantize_dm_f32's mbits_dev): an MSE estimator's vote for a quantizer
 * whose sign is still that flag.  n_bits <= 8 (both signs' widths 1 .. n_bits - sign_bits travel by value). */
int fp8q_quantize_dms_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                          const float *mbits_dev, int n_bits, const unsigned char *signed_flag, fp8q_stream_t stream);

/*
 * One calibration step of a quantizer whose range comes from FP_MSE_Estimator, in ONE call:
 * QuantizationManager.forward in estimate_ranges state (quantization/quantization_manager.py:114-122) around
 * FP_MSE_Estimator.forward (quantization/range_estimators.py:318-369) --
 *   first != 0   row max|x| -> search grid linspace(0.1 max|x|, 1.2 max|x|, n_cand) per row; this batch's table entries are
 *                written instead of added (the table need not be cleared beforehand)                            (:295-316)
 *   always       mses[n_m, n_cand, C] += row-mean((x - q(x; mbits[m], grid[i, c]))^2)   (fp8q_mse_grid_f32)   (:337-347)
 *                vote of the mantissa width, per-row argmin -> state.mbits / vote / maxval / xmin (fp8q_mse_select_f32) (:350-369)
 *   y != NULL    y = quantize(x; maxval, voted width)  (fp8q_quantize_f32 when n_m == 1, else fp8q_quantize_dm_f32).  For a
 *                per-tensor quantizer (C == 1, x and y 16-byte co-aligned) vote + argmin ride in the prologue of this K1 launch
 *                instead of a launch of their own: same outputs in state.mbits / vote / maxval / xmin, same y.
 * Everything is enqueued on `stream`; nothing comes back to the host.  The state is caller-owned device memory
 * (any layout; the torch host allocates one block per estimator) and persists between the batches of a calibration.
 * Workspaces: ws_minmax as fp8q_minmax_f32 (zeroed, left zero; only read when first != 0), ws_select as fp8q_mse_select_f32
 * (zero header), ws_mse as fp8q_mse_grid_f32; fp8q_mse_calibrate_workspace_bytes returns the last size and writes the other two.
 * Results are those of the four entry points called one after the other (bit for bit).
 * pre != NULL (per-tensor quantizers, C == 1, inner == N * C * HW of pre): the quantizer sits behind a batch norm + activation
 * (+ residual); `x` is then a caller-owned scratch of `inner` floats that RECEIVES t = act(bn(pre->x) + residual) -- written by
 * fp8q_affine_act_minmax_linspace_f32 (first batch: abs-max and grid from the same launch) or fp8q_affine_act_f32 -- and the
 * search / quantization run on it: quantized_folded_bn.py:39-55 + quantization_manager.py:114-122 in one call.
 * ws_minmax then needs max(fp8q_minmax_workspace_bytes, fp8q_affine_act_minmax_workspace_bytes) bytes.
 */
typedef struct fp8q_affine_pre {
    const float *x;          /* [N, C, HW] the producer's output (convolution / linear) */
    const float *residual;   /* [N, C, HW] or NULL */
    const float *alpha_beta; /* folded [C, 2] batch-norm vector (fp8q_bn_fold_f32) or NULL */
    int64_t N, C, HW;
    int act;                 /* 0 none, 1 ReLU, 2 ReLU6 */
} fp8q_affine_pre;
typedef struct fp8q_mse_state {
    float *cur_min, *cur_max; /* [C] row minimum / maximum of the first batch */
    float *absmax;            /* [C] max|x| of the first batch: defines the grid */
    float *grid;              /* [n_cand, C] */
    float *mses;              /* [n_m, n_cand, C], accumulated over the batches */
    float *maxval;            /* [C] the winner's clipping value (what set_quant_range(xmin, maxval) stores) */
    float *xmin;              /* [C] -sign_bits * maxval; may be NULL */
    float *mbits;             /* [1] voted mantissa width */
    int *vote;                /* [1] its index in mbits_host; may be NULL */
} fp8q_mse_state;
size_t fp8q_mse_calibrate_workspace_bytes(int64_t C, int64_t inner, int64_t n_cand, int n_m, size_t *minmax_bytes,
                                          size_t *select_bytes);
int fp8q_mse_calibrate_f32(float *x, float *y, int64_t C, int64_t inner, const fp8q_mse_state *state, int first,
                           int n_cand, const float *mbits_host, int n_m, int n_bits, int sign_bits, const fp8q_affine_pre *pre,
                           void *ws_minmax, size_t ws_minmax_bytes, void *ws_select, size_t ws_select_bytes, void *ws_mse,
                           size_t ws_mse_bytes, fp8q_stream_t stream);

/*
 * The float64 lane -- BASELINE config 1.  compute_quant_error.py:19-20 draws float64 samples; LineSearchEstimator
 * (quantization/range_estimators.py:161-169, 205-222, 236-256) takes their min / max and scores 1000 clipping candidates
 * on them, and quant_error_estimator.py:67-73 runs the quantizer's forward on a float64 sample.  Under ATen's type
 * promotion quantize_to_fp8_ste_MM (fp8_quantizer.py:105-133) then keeps M, E and bias in float32 (maxval and the mantissa
 * bits are float32 tensors) and evaluates everything downstream of x in float64.  Arithmetic contract: bit-identical to
 * oracle/fp8q_oracle.c:orc_quant1_f64 (double log2 / 2^x = the table-driven 1-ulp evaluations defined there; against the
 * reference's own 1-ulp Sleef routines: <= 2 ulp(double) per element, the same grid point -- tests/golden/g1c_*.npz).
 *   fp8q_quantize_f64   K1: x, y [C, inner] float64 (y may alias x), 8-byte aligned; maxval fp32 [1] or [C].  16 B / element.
 *   fp8q_minmax_f64     row_min / row_max [C] float64 of x [C, inner] (NaN anywhere in a row -> NaN); two launches.
 *   fp8q_mse_grid_f64   K4: out[n_m, n_cand, C] (float64) += sum over the row of (x - q(x; mbits[m], grid[i, c]))^2
 *                       (reduce_sum != 0: LineSearchEstimator.loss_fx, torch.sum) or its mean (reduce_sum == 0:
 *                       FP_MSE_Estimator.forward :337-347).  Per element the K1-f64 arithmetic, bit for bit; the sums
 *                       are formed in another order than ATen's (or the oracle's compensated one): ~1e-15 relative.
 *                       ws: at least fp8q_mse_f64_workspace_bytes() bytes, 8-byte aligned, need not be initialised.
 */
int fp8q_quantize_f64(const double *x, double *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                      float mbits, int n_bits, int sign_bits, fp8q_stream_t stream);
size_t fp8q_minmax_f64_workspace_bytes(int64_t C, int64_t inner);
int fp8q_minmax_f64(const double *x, int64_t C, int64_t inner, double *row_min, double *row_max, void *ws,
                    size_t ws_bytes, fp8q_stream_t stream);
size_t fp8q_mse_f64_workspace_bytes(int64_t C, int64_t inner, int64_t n_cand, int n_m);
int fp8q_mse_grid_f64(const double *x, int64_t C, int64_t inner, const float *grid, int64_t n_cand,
                      const float *mbits_host, int n_m, int n_bits, int sign_bits, double *out, int reduce_sum, void *ws,
                      size_t ws_bytes, fp8q_stream_t stream);

/*
 * N2 -- producer epilogue fused with the activation quantizer: eval-mode batch norm
 * (NCHW, per-channel mean / invstd = 1/sqrt(var+eps) / gamma / beta, all four NULL to skip),
 * + optional residual add, + optional activation (act: 0 none, 1 ReLU, 2 ReLU6), then the
 * per-tensor FP8 quantizer -- BNFusedHijacker.forward, quantization/quantized_folded_bn.py:39-55,
 * and the residual tail of models/resnet_quantized.py:43-46, in one pass (8 B / element, 12 with a residual).
 * The _minmax twin produces the range of the same pre-quantization tensor for calibration
 * (same fold semantics as fp8q_minmax_f32; ws of at least fp8q_affine_act_minmax_workspace_bytes(N, C, HW)
 * bytes).  x, residual, y: [N, C, HW] fp32, 16-byte aligned;
 * C*HW must be a multiple of 4 (FP8Q_EUNSUPPORTED otherwise: use the unfused calls).
 */
int fp8q_affine_act_quantize_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C,
                                 int64_t HW, const float *mean, const float *invstd, const float *gamma,
                                 const float *beta, int act, const float *maxval, float mbits, int n_bits,
                                 int sign_bits, fp8q_stream_t stream);
/*
 * The same epilogue with the batch norm's per-channel constants folded once: fp8q_bn_fold_f32 writes
 * alpha_beta[c] = {alpha_c, beta'_c} = {invstd_c * gamma_c, fma(-mean_c, alpha_c, beta_c)} ([C, 2] fp32, 8-byte aligned) --
 * the two numbers the kernels above form per plane -- and fp8q_affine_act_quantize_ab_f32 reads them (one 8-byte load
 * per plane instead of four 4-byte ones).  Bit-identical results; in eval mode the vector changes only when the BN
 * parameters do, so a caller folds once and reuses it for every forward.
 */
int fp8q_bn_fold_f32(const float *mean, const float *invstd, const float *gamma, const float *beta, int64_t C,
                     float *alpha_beta, fp8q_stream_t stream);
/*
 * A per-tensor quantizer whose range is FIXED can also be prepared once: fp8q_quantizer_prepare_f32 writes the channel
 * constants and the {s, 1/s} table every launch otherwise rebuilds from maxval (FP8Q_PREP_BYTES bytes, 16-byte aligned,
 * device memory).  Passed as `prep` (NULL = rebuild), it takes 0.5-1 us off the critical path of launches on cache-sized
 * activations (4-10 us each: most of a ResNet-18 / MobileNetV2 forward's quantizer launches).  `prep` must have been
 * prepared from the same maxval VALUE, mbits, n_bits and sign_bits as the call it is passed to; results are bit-identical.
 * alpha_beta may be NULL in the _ab entry point (no batch norm: the residual tails).
 */
#define FP8Q_PREP_BYTES 1056 /* float4 {maxval, lo, bias, threshold} + 130 x float2 {s_p, 1 / s_p} */
int fp8q_quantizer_prepare_f32(const float *maxval, float mbits, int n_bits, int sign_bits, float *prep, fp8q_stream_t stream);
int fp8q_affine_act_quantize_ab_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW,
                                    const float *alpha_beta, int act, const float *maxval, const float *prep, float mbits,
                                    int n_bits, int sign_bits, fp8q_stream_t stream);

/* The epilogue WITHOUT the quantizer: y = act(bn(x) + residual) (same kernels, same BN arithmetic, the quantizer switched off).
 * What an MSE range estimator behind a BN + activation searches on during calibration (quantized_folded_bn.py:39-55 followed by
 * range_estimators.py:318-369): one 8 B / element pass instead of torch's batch_norm + activation passes.  alpha_beta: the folded
 * [C, 2] vector of fp8q_bn_fold_f32, or NULL (no batch norm). */
int fp8q_affine_act_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW, const float *alpha_beta,
                        int act, fp8q_stream_t stream);
/*
 * Which kernel the three quantizing entries above (fp8q_affine_act_quantize_f32, _ab_, fp8q_affine_act_f32) launch for an
 * [N, C, HW] tensor, with (has_bn 1 or 2) or without (0) a batch norm, at the process's settings.  Host arithmetic only: no
 * launch, no device -- the launcher's own argument block and dispatch with a callback that records, so that a test can assert
 * the route before it trusts a shape.  kernel: FP8Q_AFFINE_* below (-1 with launches == 0 when N == 0); direct: a staged
 * kernel behind a batch norm keeps the constants of a piece's planes in registers (at most two planes per piece) instead of
 * staging them in LDS; cpp: most planes one 4096-element piece overlaps; launches: one per 65535 images; grid_x / grid_y: of
 * the first launch.  Errors as the entries report them for the shape: FP8Q_EINVAL (N < 0, C or HW not positive, has_bn
 * outside 0..2, info NULL), FP8Q_EUNSUPPORTED (C * HW not a multiple of 4, C * HW >= 2^31, HW >= 2^24, C * HW * HW >= 2^48);
 * `info` is written on FP8Q_OK only.
 */
#define FP8Q_AFFINE_STAGED_NT 0 /* k_affine_act<true, 4>: 16 KiB pieces, nontemporal (tensors of 64 MiB and more) */
#define FP8Q_AFFINE_SMALL 1     /* k_affine_act_small: one 16-byte group per lane */
#define FP8Q_AFFINE_STAGED1 2   /* k_affine_act<false, 1>: HW < 4 behind a batch norm */
#define FP8Q_AFFINE_STAGED4 3   /* k_affine_act<false, 4>: only with FP8Q_EPI_SMALL_M below the nontemporal threshold */
typedef struct fp8q_affine_route_info {
    int kernel;
    int direct;
    int cpp;
    int launches;
    int64_t grid_x, grid_y;
} fp8q_affine_route_info;
int fp8q_affine_act_route(int64_t N, int64_t C, int64_t HW, int has_bn, fp8q_affine_route_info *info);
/* The same pass for the FIRST calibration batch of an MSE estimator: t = act(bn(x) + residual) is written AND its minimum /
 * maximum / abs-max and the search grid linspace(lo_frac * max|t|, hi_frac * max|t|, n_cand) ([n_cand, 1]) come out of the same
 * launch (what fp8q_affine_act_f32 + fp8q_minmax_linspace_f32 on t give, bit for bit; 8 B / element instead of 12).
 * ws: as fp8q_affine_act_minmax_f32 (zeroed, left zero; fp8q_affine_act_minmax_workspace_bytes). */
int fp8q_affine_act_minmax_linspace_f32(const float *x, const float *residual, float *t, int64_t N, int64_t C, int64_t HW,
                                        const float *alpha_beta, int act, float *cur_min, float *cur_max, float *maxval_out,
                                        float *grid, int n_cand, double lo_frac, double hi_frac, void *ws, size_t ws_bytes,
                                        fp8q_stream_t stream);
size_t fp8q_affine_act_minmax_workspace_bytes(int64_t N, int64_t C, int64_t HW);
int fp8q_affine_act_minmax_f32(const float *x, const float *residual, int64_t N, int64_t C, int64_t HW,
                               const float *mean, const float *invstd, const float *gamma, const float *beta,
                               int act, float *cur_min, float *cur_max, float *maxval_out, int fold_mode,
                               double momentum, int first, void *ws, size_t ws_bytes, fp8q_stream_t stream);

int fp8q_affine_act_minmax_packed_f32(const float *x, const float *residual, int64_t N, int64_t C, int64_t HW,
                                      const float *mean, const float *invstd, const float *gamma, const float *beta,
                                      int act, float *cur_min, float *cur_max, float *maxval_out, float *packed,
                                      int fold_mode, double momentum, int first, void *ws, size_t ws_bytes,
                                      fp8q_stream_t stream);

/*
 * N3 -- real FP8 storage codes.  The reference only simulates the format; its
 * enumerator generate_all_values_fp (fp8_quantizer.py:13-41) defines the byte layout
 * [sign | E exponent bits | M fraction bits] (exponent code 0 subnormal, no inf/NaN codes).
 *   fp8q_encode_u8: codes[i] = the byte whose value is quantize_to_fp8_ste_MM(x)[i]
 *   fp8q_decode_u8: y[i] = value of codes[i].  decode(encode(x)) == fp8q_quantize_f32(x) bit for bit whenever
 *                   the channel's scales are exactly geometric in fp32 (s_(p+1) == 2 s_p: true for every range
 *                   with |k - bias| below bias's binade, e.g. all weight-sized ranges); otherwise an element
 *                   that rounds UP into the next binade is 2^(M+1) s_p in K1 and 2^M s_(p+1) after decoding,
 *                   two fp32 renderings of the same grid point that can differ by ulp(k - bias) ln 2 relative (a few ULP, <= 5e-6 for |bias| < 100; the reference has the
 *                   same ambiguity: it emits either, depending on which side x came from)
 * n_bits <= 8 and at least one exponent bit (FP8Q_EUNSUPPORTED otherwise).  The format has no NaN: NaN inputs and degenerate channels (maxval 0/inf/NaN, whose
 * K1 output is NaN) encode as 0.  HBM traffic: 5 B / element each.
 * fp8q_decode_u8 expects codes below 2^n_bits: what a byte with a bit at or above n_bits decodes to is not defined.
 */
int fp8q_encode_u8(const float *x, uint8_t *codes, int64_t C, int64_t inner, const float *maxval,
                   int64_t n_maxval, float mbits, int n_bits, int sign_bits, fp8q_stream_t stream);
int fp8q_decode_u8(const uint8_t *codes, float *y, int64_t C, int64_t inner, const float *maxval,
                   int64_t n_maxval, float mbits, int n_bits, int sign_bits, fp8q_stream_t stream);

/*
 * Which kernel fp8q_encode_u8 (encode != 0) or fp8q_decode_u8 (encode == 0) launches for a [C, inner] tensor of a format, at
 * the process's settings.  Host arithmetic only: no launch, no device -- the entries' own code behind their argument checks,
 * the launchers' geometry and dispatch included, with a callback that records instead of launching, so that a test can assert
 * the route before it trusts a shape.  n_maxval: C (one range per row) or 1 (one for the tensor: the entries then see one row
 * of C * inner elements).  fp_mod16 / code_mod16: the addresses of the float32 side (x or y; a multiple of 4) and of the codes
 * modulo 16.
 *   kernel          FP8Q_CODEC_K_* below; -1 with launches == 0 for an empty tensor
 *   nontemporal     the instance for tensors of 64 MiB and more
 *   nch             k_rows_flat: chunks of 4096 elements per tile, 1..4
 *   wide            k_rows_flat, encode: the codes start on a 16-byte boundary, four groups of a lane leave as one 16-byte store
 *                   (else as dwords)
 *   grid_x, grid_y  of the first launch
 *   launches        k_codec_rows: one per slab of 65535 rows; k_rows_flat: 1
 *   steps           k_codec_rows: grid-stride steps of a block over its row's 4096-element pieces, ceil(pieces / grid_x);
 *                   k_rows_flat: tiles a block walks (more than 1 beyond 32768 tiles)
 * k_codec_rows picks its vector width per row from the row's own addresses: 16-byte float32 accesses need that side 16-byte
 * aligned and the codes 4-byte aligned (encode: 16-byte aligned, else every element goes alone); otherwise scalar.
 * Fields that do not apply to the kernel are 0.  Errors as the entries report them for the shape and format: FP8Q_EINVAL (a
 * negative size, n_maxval neither 1 nor C, n_bits < 2, sign_bits not 0 or 1, a NaN mbits; here also a phase out of range or info NULL),
 * FP8Q_EUNSUPPORTED (n_bits > 8, no exponent bit, more than seven); `info` is written on FP8Q_OK only.
 */
#define FP8Q_CODEC_K_ROWS_FLAT 0    /* k_rows_flat: per-channel rows of 4..2047 elements whose tables fit, fp32 side 16-byte and codes 4-byte aligned */
#define FP8Q_CODEC_K_CODEC_ROWS 1   /* k_codec_rows: one row per blockIdx.y; everything else */
typedef struct fp8q_codec_route_info {
    int kernel;
    int nontemporal;
    int nch;
    int wide;
    int launches;
    int reserved;
    int64_t grid_x, grid_y, steps;
} fp8q_codec_route_info;
int fp8q_codec_route(int encode, int64_t C, int64_t inner, int64_t n_maxval, float mbits, int n_bits, int sign_bits,
                     int fp_mod16, int code_mod16, fp8q_codec_route_info *info);

/*
 * The launch geometry of the chunked kernels: the INT quantizers (fp8q_int_quantize_* / fp8q_int_range_quantize_*), the INT
 * codes (fp8q_int_to_integer_f32, fp8q_int_encode*, fp8q_int_decode*) and the hardware FP8 lane (fp8q_ocp_*), which all give
 * one aligned 4096-element chunk to a block and keep the constants of the rows overlapping it in dynamic LDS.  Host arithmetic
 * only: no launch, no device -- the entries' own argument check, geometry, sign rule and launch plan, so that a test can
 * assert the route before it trusts a shape.
 *   C, inner, n_range   the tensor and its range vector, as the entries take them (n_range: 1 or C)
 *   elem_bytes          of the streamed value tensor: 4, or 2 for the INT kernels on fp16 / bf16 tensors
 *   in_mod16, out_mod16 the addresses of the launch's input and output modulo 16 (fp8q_int_decode's VEC instance is content
 *                       with codes on a multiple of 4 bytes, 8 for 2-byte codes: pass 0 for such an address)
 *   symmetric, sets_range   the quantizer's kind, and whether the launch sets the range (fp8q_int_range_quantize_*)
 * Reported:
 *   grid_x          blocks: chunks of the tensor
 *   per_channel     n_range > 1; per tensor the kernels see one row
 *   rows_per_chunk  LDS entries of a block: min(4096 / inner + 2, C), 1 per tensor
 *   lds_bytes       16 * rows_per_chunk of dynamic LDS (above 64 KiB when inner == 1 and C > 4096)
 *   magic           the multiplier that finds an element's row: floor(2^32 / inner) + 1; 0 when inner == 1 or per tensor
 *   two_row         inner >= 4096: a chunk overlaps at most two rows and no division is made
 *   vec             the 16-byte instance: both addresses 16-byte aligned, elem_bytes == 4 (the half kernels walk from x's own
 *                   16-byte boundary instead)
 *   nontemporal     the instance for tensors of 64 MiB and more (fp8q_int_encode_h16 / fp8q_int_decode_h16 have none)
 *   sign_prepass    a range-setting symmetric launch of more than 2048 rows: k_int_sign folds the sign first; otherwise every
 *                   block folds it itself
 *   last_chunk      elements of the last chunk, 1..4096
 * Errors as the entries report them for the shape: FP8Q_EINVAL (a size <= 0, n_range neither 1 nor C, a per-channel row or a
 * chunk count beyond 32 bits; here also elem_bytes, a phase out of range or info NULL); `info` is written on FP8Q_OK only.
 */
typedef struct fp8q_chunk_route_info {
    int per_channel;
    int rows_per_chunk;
    int two_row;
    int vec;
    int nontemporal;
    int sign_prepass;
    uint32_t magic;
    int reserved;
    int64_t grid_x, lds_bytes, last_chunk;
} fp8q_chunk_route_info;
int fp8q_chunk_route(int64_t C, int64_t inner, int64_t n_range, int elem_bytes, int in_mod16, int out_mod16, int symmetric,
                     int sets_range, fp8q_chunk_route_info *info);

/*
 * Multi-tensor K1 -- all weight tensors of a model in one launch: the reference quantizes
 * each layer's weight in that layer's forward (hijacker.py:70-108 -> quantize_weights), 21 tiny launches
 * for ResNet-18; with fixed ranges they are independent and can be enqueued together.
 *   descs  HOST array of n descriptors (read during the call only); every field as in fp8q_quantize_f32
 * Tensors are batched 32 per launch; a tensor that cannot be batched (pointers not 16-byte aligned, rows
 * shorter than 4 or too short for per-row tables, >= 64 MiB) gets its own fp8q_quantize_f32 launch, in order.
 * Results are bit-identical to n separate fp8q_quantize_f32 calls.  Nothing is enqueued if a descriptor is bad.
 */
typedef struct fp8q_tensor_desc {
    const float *x;
    float *y;
    const float *maxval;
    int64_t C, inner, n_maxval;
    float mbits;
    int n_bits, sign_bits;
} fp8q_tensor_desc;
int fp8q_multi_quantize_f32(const fp8q_tensor_desc *descs, int n, fp8q_stream_t stream);

/*
 * Multi-tensor K2+K5+K1 -- all weight tensors of a model in ESTIMATE state (per-channel current_minmax with
 * set_maxval: QuantizationManager.forward, quantization_manager.py:114-122, once per layer in the reference): one launch
 * finds every row's range and writes maxval_out[i][c] = |max(|min_c|, max_c)| ([C] floats per tensor, a HOST array of n
 * device pointers), a second one is fp8q_multi_quantize_f32 reading those ranges.  descs[i].n_maxval must equal C;
 * descs[i].maxval is an INPUT field and is not written: it must be NULL or name the same buffer as maxval_out[i]
 * (FP8Q_EINVAL otherwise -- a range buffer elsewhere would be ignored).  Two launches for a whole model instead of one
 * per layer; results bit-identical to fp8q_minmax_quantize_f32 per tensor.  This is what a rank of the channel-sharded
 * multi-GPU weight path runs on its shards before the all-gather (fp8q.dist.quantize_weights_sharded_bucketed).
 */
int fp8q_multi_minmax_quantize_f32(const fp8q_tensor_desc *descs, float *const *maxval_out, int n, fp8q_stream_t stream);
/*
 * Storage codes (fp8q_encode_u8 / fp8q_decode_u8) for many tensors at once: what the bucketed all-gather of channel-sharded
 * weights puts on the wire -- 1 byte per element instead of 4.  Same descriptor table; the CODE side is typed through the
 * float pointers of fp8q_tensor_desc:  _encode_: x = fp32 values (16-byte aligned), y = (float *) of the uint8 codes
 * (4-byte aligned);  _decode_: x = (const float *) of the codes, y = fp32 values.  Other alignments take one
 * fp8q_encode_u8 / fp8q_decode_u8 call per tensor.  _minmax_encode_: per-channel current_minmax ranges first
 * (maxval_out, as fp8q_multi_minmax_quantize_f32), then the codes: two launches for a whole bucket.
 * Bit-identical to the single-tensor entry points; n_bits <= 8 and at least one exponent bit (FP8Q_EUNSUPPORTED otherwise).
 */
int fp8q_multi_encode_u8(const fp8q_tensor_desc *descs, int n, fp8q_stream_t stream);
int fp8q_multi_minmax_encode_u8(const fp8q_tensor_desc *descs, float *const *maxval_out, int n, fp8q_stream_t stream);
int fp8q_multi_decode_u8(const fp8q_tensor_desc *descs, int n, fp8q_stream_t stream);

/*
 * Prepared multi-tensor launch.  fp8q_multi_quantize_f32 validates, classifies and packs its descriptors on every
 * call; for a fixed set of tensors (a model's weights after fix_ranges(), re-quantized whenever the weights change)
 * that work is done ONCE here and a call costs one kernel launch per 32 tensors.  The plan is a small HOST object
 * (the only allocation this library ever makes; no device memory); it records pointers, so the tensors must stay
 * where they are and keep their shapes -- their CONTENTS (weights, ranges) may change between launches.
 *   create    0 and *plan on success; a negative FP8Q_E* / positive hipError_t (out of host memory) otherwise
 *   launch    bit-identical to fp8q_multi_quantize_f32 on the same descriptors; enqueue-only; thread-safe
 *   launches  kernel launches one fp8q_multi_plan_launch enqueues
 */
typedef struct fp8q_multi_plan fp8q_multi_plan;
int fp8q_multi_plan_create(const fp8q_tensor_desc *descs, int n, fp8q_multi_plan **plan);
int fp8q_multi_plan_launch(const fp8q_multi_plan *plan, fp8q_stream_t stream);
int fp8q_multi_plan_launches(const fp8q_multi_plan *plan);
void fp8q_multi_plan_destroy(fp8q_multi_plan *plan);

/*
 * Which launch serves each tensor of a multi-tensor call -- host only, nothing is enqueued: the plan that
 * fp8q_multi_quantize_f32 (mode 0), fp8q_multi_encode_u8 (mode 3) or fp8q_multi_decode_u8 (mode 4) would build from these
 * descriptors (the same function builds it, pointers included: their alignment decides), reported per descriptor.
 *   step_of  [n] the plan step (launch, in order) the tensor landed in; -1 for an empty tensor, which gets none
 *   batched  [n] 1: that step is the batched kernel, shared with up to 31 other tensors; 0: the tensor's own single-tensor
 *            launch (misaligned pointers, fewer than 4 elements, 2^31 elements or more, rows shorter than 4 or longer than
 *            60000 elements, per-row tables of one 4096-element chunk beyond 36 KiB, 64 MiB or more); -1: empty
 *   n_steps  launches of the whole call
 * Errors are the launch's own (FP8Q_EINVAL / FP8Q_EUNSUPPORTED for a bad descriptor); a mode outside {0, 3, 4} or a NULL
 * output is FP8Q_EINVAL.  The tests assert it before they compare (tests/test_multi_routes.py).
 */
int fp8q_multi_route(const fp8q_tensor_desc *descs, int n, int mode, int *step_of, int *batched, int *n_steps);

/* Plain float4 copy kernel with the same launch shape as K1: the measured HBM ceiling that
 * bench.py reports next to the 8 TB/s spec figure. */
int fp8q_copy_f32(const float *x, float *y, int64_t n, fp8q_stream_t stream);

/*
 * Uniform (INT) fake-quantization (csrc/fp8q_int.hip): the reference's AsymmetricUniformQuantizer /
 * SymmetricUniformQuantizer (uniform_quantizers.py) in the linear scale domain, bit for bit its fp32 op chain:
 *   y = scale * (clamp(rint(x / scale) + zp, int_min, int_max) - zp),  scale = max(delta, eps),
 *   zp = clamp(rint(zero_float), int_min, int_max) (asymmetric) or 0 (symmetric).
 * Asymmetric: [int_min, int_max] = [0, 2^n - 1].  Symmetric: [-2^(n-1), 2^(n-1) - 1] when the device byte
 * signed_flag[0] is non-zero, [0, 2^n - 1] otherwise -- read by the kernels, never by the host.
 * x, y [C, inner] fp32; delta / zero_float / x_min / x_max have n_delta (n_range) elements, 1 (per tensor) or C (per
 * channel, dim 0).  zero_float is unused (may be NULL) when symmetric; signed_flag is unused (may be NULL) when not.
 * n_bits in [2, 16] (FP8Q_EUNSUPPORTED otherwise); FP8Q_EINVAL for null pointers, empty shapes, n_delta not in {1, C}.
 * HBM traffic: 8 B / element.  Enqueue-only.
 *
 *   int_quantize       fixed ranges: one launch.
 *   int_set_range      (x_min, x_max) [n] -> delta, zero_float (asymmetric), signed_flag (symmetric: the sign of the
 *                      whole vector, NaN -> unsigned): x_min' = min(x_min, 0), x_max' = max(x_max, eps),
 *                      delta = (x_max' - x_min') / int_max, zero_float = -x_min' / delta, or, symmetric,
 *                      delta = max(|x_min'|, x_max') / int_max.  One launch (two for more than 2048 symmetric channels).
 *   int_range_quantize int_set_range and int_quantize in ONE launch (two for more than 2048 symmetric channels).
 *   int_minmax_quantize per-channel current_minmax: row_min / row_max [C] (fp8q_minmax_f32, FOLD_CURRENT; ws / ws_bytes
 *                      as there), then int_range_quantize on them.  Two launches (three beyond 2048 symmetric channels).
 */
int fp8q_int_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *delta,
                          const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                          int symmetric, float eps, fp8q_stream_t stream);
int fp8q_int_set_range_f32(const float *x_min, const float *x_max, int64_t n, float *delta, float *zero_float,
                           unsigned char *signed_flag, int n_bits, int symmetric, float eps, fp8q_stream_t stream);
int fp8q_int_range_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *x_min,
                                const float *x_max, int64_t n_range, float *delta, float *zero_float,
                                unsigned char *signed_flag, int n_bits, int symmetric, float eps,
                                fp8q_stream_t stream);
int fp8q_int_minmax_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, float *row_min, float *row_max,
                                 float *delta, float *zero_float, unsigned char *signed_flag, int n_bits, int symmetric,
                                 float eps, void *ws, size_t ws_bytes, fp8q_stream_t stream);

/*
 * N2 for the uniform (INT) quantizers (csrc/fp8q_intepilogue.hip): the producer epilogue of fp8q_affine_act_f32 fused with the
 * per-tensor INT quantizer above, in one pass (8 B / element, 12 with a residual):
 *   t = fma(x, alpha_c, beta'_c)     alpha_beta: the folded [C, 2] vector of fp8q_bn_fold_f32, or NULL (no batch norm)
 *   t = t + residual                 residual NULL: skipped
 *   t = relu(t) / relu6(t)           act: 0 none, 1 ReLU, 2 ReLU6; NaN stays NaN
 *   y = scale * (clamp(rint(t / scale) + zp, int_min, int_max) - zp)
 * Bit for bit fp8q_int_quantize_f32 (n_delta = 1) applied to the output of fp8q_affine_act_f32, NaN positions, +-inf and -0
 * included.  x, residual, y: [N, C, HW] fp32, 16-byte aligned; y may alias x or residual.  The quantizer is per tensor:
 * delta, zero_float (asymmetric; unused and may be NULL when symmetric) and x_min, x_max have ONE element; the symmetric sign
 * is the device byte signed_flag[0] (unused and may be NULL when not symmetric).
 *   fp8q_int_affine_act_quantize_f32        fixed ranges.
 *   fp8q_int_affine_act_range_quantize_f32  set_quant_range(x_min[0], x_max[0]) and the quantizer in the same launch, as
 *       fp8q_int_range_quantize_f32: every block derives the range, one block writes delta_out[0], zero_float_out[0]
 *       (asymmetric) and signed_flag_out[0] (symmetric).  As there, the three outputs must not overlap x_min, x_max, x,
 *       residual or y (other blocks still read those).
 * FP8Q_EINVAL: a null or misaligned pointer (x, residual, y: 16 bytes; alpha_beta: 8), act outside 0..2, C or HW not
 * positive.  FP8Q_EUNSUPPORTED: C * HW not a multiple of 4, C * HW >= 2^31, HW >= 2^24, C * HW * HW >= 2^48, n_bits outside
 * [2, 16].  N == 0: nothing is launched.  One launch per 65535 images.  Enqueue-only.
 */
int fp8q_int_affine_act_quantize_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW,
                                     const float *alpha_beta, int act, const float *delta, const float *zero_float,
                                     const unsigned char *signed_flag, int n_bits, int symmetric, float eps,
                                     fp8q_stream_t stream);
int fp8q_int_affine_act_range_quantize_f32(const float *x, const float *residual, float *y, int64_t N, int64_t C, int64_t HW,
                                           const float *alpha_beta, int act, const float *x_min, const float *x_max,
                                           float *delta_out, float *zero_float_out, unsigned char *signed_flag_out, int n_bits,
                                           int symmetric, float eps, fp8q_stream_t stream);

/*
 * Integer codes of the uniform (INT) quantizers (csrc/fp8q_intcodec.hip): the storage form of the lane above, and the
 * reference's to_integer_forward (uniform_quantizers.py:108-133).  With scale, zp, int_min, int_max as above (the symmetric
 * sign read from signed_flag[0] on the device):
 *   t = clamp(rint(x / scale) + zp, int_min, int_max)      in fp32, every op rounded on its own
 *   fp8q_int_to_integer_f32   t as float32.  NaN stays NaN.  A zero level is +0, as torch's CUDA chain gives it (its clamp
 *                             turns the -0 of -0 + -0, possible only with a zero_float of -0, into +0; the CPU clamp keeps it).
 *   fp8q_int_encode           t as an integer: ONE byte per element for n_bits <= 8, TWO bytes (little endian) for 9..16,
 *                             holding the two's-complement low bits of t: unsigned ranges store 0 .. 2^n - 1, the signed
 *                             symmetric range -2^(n-1) .. 2^(n-1) - 1.  NaN has no code: it stores the code of the value 0,
 *                             which is zp (asymmetric) or 0 (symmetric), as fp8q_encode_u8 stores 0; a channel whose zp is
 *                             itself NaN (a NaN zero_float) stores 0.
 *   fp8q_int_decode           y = scale * (float(code) - zp); the code is read as signed exactly when the quantizer is
 *                             symmetric and signed_flag[0] is non-zero.
 * decode of encode equals fp8q_int_quantize_f32 bit for bit on every element whose x is not NaN -- +-inf inputs and channels
 * whose delta is 0, inf or NaN included: both sides run the same last two operations on the same exactly representable
 * integer.  encode equals to_integer cast to the storage type wherever to_integer is not NaN.  to_integer equals the eager
 * to_integer_forward chain bit for bit on the same range buffers.
 * Arguments and error codes as fp8q_int_quantize_f32: FP8Q_EINVAL for null pointers, empty shapes, n_delta not in {1, C};
 * FP8Q_EUNSUPPORTED for n_bits outside [2, 16].  codes [C, inner] must be aligned to its element size (FP8Q_EINVAL); the
 * 16-byte paths need x / y and codes 16-byte aligned (decode: codes aligned to 4 elements), other alignments go element by
 * element.  HBM traffic: encode and decode 5 B / element (6 B with 2-byte codes), to_integer 8 B.  One launch, no workspace,
 * enqueue-only.
 */
int fp8q_int_to_integer_f32(const float *x, float *t, int64_t C, int64_t inner, const float *delta,
                            const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                            int symmetric, float eps, fp8q_stream_t stream);
int fp8q_int_encode(const float *x, void *codes, int64_t C, int64_t inner, const float *delta, const float *zero_float,
                    int64_t n_delta, const unsigned char *signed_flag, int n_bits, int symmetric, float eps,
                    fp8q_stream_t stream);
int fp8q_int_decode(const void *codes, float *y, int64_t C, int64_t inner, const float *delta, const float *zero_float,
                    int64_t n_delta, const unsigned char *signed_flag, int n_bits, int symmetric, float eps,
                    fp8q_stream_t stream);

/*
 * The line search of the uniform quantizers (csrc/fp8q_int.hip): LineSearchEstimator's candidates
 * (range_estimators.py:161-169, 236-256) in ONE pass over the data instead of one quantizer pass per candidate.
 *   out[k, c] += sum over row c of (x - q_k(x))^2,   k < n_cand, c < C
 * with q_k the uniform quantizer after set_quant_range(one_sided ? 0 : -thr[k, c], thr[k, c]): the range chain above in
 * fp32 on that one-element range (symmetric: signed iff its x_min < 0), then the quantize chain.
 *   x    [C, inner] contiguous float32 (_f32) or float64 (_f64), natural alignment: views at any element offset.
 *   thr  [n_cand, C] fp32 (what torch.tensor(pos_thr).float() holds);  out [n_cand, C] float64, ACCUMULATED.
 * Per element, _f32: the fp32 chain bit for bit, d = x - y and d * d in fp32, summed in float64.  _f64: ATen's type
 * promotion -- scale and zero point are fp32 values widened exactly; the IEEE double division x / scale, rint, + zp, the
 * clamp, scale * (r - zp), x - y and the square in float64.  No contraction.  A NaN in a row makes the row's sums NaN.
 * The sums have a fixed order and use no atomics: two calls on the same buffers give the same bits; against the exact sum
 * of the squares the relative error is below (inner + 2) 2^-53.
 * ws: at least fp8q_int_sse_grid_workspace_bytes() bytes, 8-byte aligned, need not be initialised.  Two launches,
 * enqueue-only, no allocation.  n_cand <= 2^20.
 * Errors, all reported before any launch: FP8Q_EINVAL for null pointers, empty shapes (C or inner <= 0), n_cand <= 0,
 * misaligned x / thr / out; FP8Q_EUNSUPPORTED for n_bits outside [2, 16]; FP8Q_ETOOMANY for C > 65535; FP8Q_EWORKSPACE
 * for a missing, misaligned or too small workspace.  FP8Q_VERSION is unchanged: the entries are additive.
 */
size_t fp8q_int_sse_grid_workspace_bytes(int64_t C, int64_t inner, int64_t n_cand);
int fp8q_int_sse_grid_f32(const float *x, int64_t C, int64_t inner, const float *thr, int64_t n_cand, int n_bits,
                          int symmetric, int one_sided, float eps, double *out, void *ws, size_t ws_bytes,
                          fp8q_stream_t stream);
int fp8q_int_sse_grid_f64(const double *x, int64_t C, int64_t inner, const float *thr, int64_t n_cand, int n_bits,
                          int symmetric, int one_sided, float eps, double *out, void *ws, size_t ws_bytes,
                          fp8q_stream_t stream);

/*
 * The half-precision lane (csrc/fp8q_h16.hip): K1, min/max and min/max + quantize on IEEE fp16 and bfloat16 tensors.
 * The reference holds maxval and the mantissa width as fp32 tensors, so ATen's type promotion widens a half x exactly,
 * runs quantize_to_fp8_ste_MM (fp8_quantizer.py:105-133) in fp32 and returns fp32.  Contract of the lane:
 *   - every input element is widened to fp32 exactly (fp16 subnormals become normal fp32 numbers, bf16 subnormals fp32
 *     subnormals; nothing is flushed; NaN stays NaN, infinities clamp like any value beyond maxval);
 *   - from there the fp32 contract applies unchanged: the fp32 result is bit-identical to fp8q_quantize_f32 -- and to
 *     oracle/fp8q_oracle.c -- on the widened input;
 *   - y_type is FP8Q_DT_F32 (the reference's promotion) or equal to x_type; in the second case the fp32 result is rounded
 *     ONCE to the storage type (round to nearest even, overflow to infinity: torch.Tensor.to(dtype)).  y may alias x then;
 *   - min/max: the fp32 minimum / maximum of the widened row with the NaN and signed-zero rules of fp8q_minmax_f32; the
 *     running estimate, the fold and maxval_out are fp32.
 * x_type / y_type: FP8Q_DT_*.  x (and a half y) need only their natural 2-byte alignment, an fp32 y 4 bytes; rows of any
 * length, views at any element offset (per channel: rows of at most 2^30 elements, C * inner below 2^42; FP8Q_EINVAL
 * beyond).  maxval fp32 [1] or [C] as in fp8q_quantize_f32.
 * Errors, all reported before any launch: FP8Q_EINVAL for null pointers, n_maxval not in {1, C}, EMPTY tensors (C or inner
 * <= 0), an x_type that is not a half type, a y_type that is neither FP8Q_DT_F32 nor x_type; FP8Q_EUNSUPPORTED for more
 * than 7 exponent bits; FP8Q_EWORKSPACE / FP8Q_ETOOLONG as in the fp32 twins.
 *   fp8q_quantize_h16         K1.  HBM traffic: 6 B / element (fp32 out), 4 B / element (half out).
 *   fp8q_minmax_h16           fp8q_minmax_f32 on half x: same arguments, same fold modes, same workspace
 *                             (fp8q_minmax_workspace_bytes(C, inner), zero on first use, left zero).  2 B / element.
 *   fp8q_minmax_quantize_h16  per-channel current_minmax + K1 (fp8q_minmax_quantize_f32 on half x): a 2 B / element scan
 *                             that writes row_min / row_max (each may be NULL) and maxval_out (REQUIRED here: it carries
 *                             the ranges to the second launch), then K1 reading maxval_out.  inner <= fp8q_fused_max_inner().
 * Enqueue-only, no allocation.  FP8Q_VERSION is unchanged: the entries are additive.
 */
#define FP8Q_DT_F32 0
#define FP8Q_DT_F16 1
#define FP8Q_DT_BF16 2
int fp8q_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *maxval,
                      int64_t n_maxval, float mbits, int n_bits, int sign_bits, fp8q_stream_t stream);
int fp8q_minmax_h16(const void *x, int x_type, int64_t C, int64_t inner, float *cur_min, float *cur_max,
                    float *maxval_out, int fold_mode, double momentum, int first, void *ws, size_t ws_bytes,
                    fp8q_stream_t stream);
int fp8q_minmax_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, float *row_min,
                             float *row_max, float *maxval_out, float mbits, int n_bits, int sign_bits,
                             fp8q_stream_t stream);

/*
 * Which kernels of the half lane a call reaches, and what its launcher chooses: the launchers' own plan code on host
 * arithmetic alone -- nothing is launched, no GPU is needed.  op: FP8Q_ROWS_QUANTIZE / _MINMAX / _MINMAX_QUANTIZE (the three
 * entries above; per_channel = 0: a per-tensor K1, for min/max the wrapper's one row [1, C * inner]; the fused entry is per
 * channel only).  x_mod16: x's address modulo 16 (even); y_type: FP8Q_DT_F32 or a half type (then x's own).  Both half types
 * take the same route.  info->n_launches kernels are described in launch order (two for the fused entry: the scan, then K1):
 *   kernel          FP8Q_H16_K_* below
 *   u, nontemporal  k_h16_quant: 16-byte groups in flight per lane (1 or 4; 4 from 2^20 groups on, unless the tables of a
 *                   chunk's rows would outgrow 40 KiB of LDS) and the instance for tensors of 64 MiB and more, which
 *                   exists for u = 4 only; k_h16_minmax_part: its nontemporal instance
 *   head, groups, tail   k_h16_quant: the scalars in front of x's first 16-byte boundary, the 16-byte groups, the scalars behind
 *   rows_per_chunk, lds_bytes   k_h16_quant: the rows a chunk of 2048 * u elements can overlap, and the bytes of their
 *                   constants and tables ((16 + 8 (pmax + 1)) each)
 *   lanes           k_h16_minmax_rows: lanes per row (1, 2, .. 64)
 *   nsplit          k_h16_minmax_part: streaming blocks per row (grid_x has the reducer block on top when nsplit > 1)
 *   grid_x, grid_y  of the first launch of this kernel
 *   launches        k_h16_minmax_part: one per slab of 65535 rows; 1 elsewhere
 * Fields that do not apply to the kernel are 0.  Errors as the entry reports them for the shape (FP8Q_EINVAL, FP8Q_EUNSUPPORTED,
 * FP8Q_ETOOLONG), FP8Q_EINVAL also for op, x_mod16 or y_type out of range and for info NULL; `info` is written on FP8Q_OK only.
 */
#define FP8Q_H16_K_QUANT 0         /* k_h16_quant: the flat range in chunks, per-row tables in LDS */
#define FP8Q_H16_K_QUANT_ROWS 1    /* k_h16_quant_rows: thread = row, no table */
#define FP8Q_H16_K_MINMAX_ROWS 2   /* k_h16_minmax_rows: per-channel rows up to 2048 elements */
#define FP8Q_H16_K_MINMAX_PART 3   /* k_h16_minmax_part: long rows, per tensor */
typedef struct fp8q_h16_launch_info {
    int kernel;
    int u;
    int nontemporal;
    int lanes;
    int nsplit;
    int rows_per_chunk;
    int launches;
    int reserved;
    int64_t head, groups, tail;
    int64_t lds_bytes;
    int64_t grid_x, grid_y;
} fp8q_h16_launch_info;
typedef struct fp8q_h16_route_info {
    int n_launches;
    int reserved;
    fp8q_h16_launch_info launch[2];
} fp8q_h16_route_info;
int fp8q_h16_route(int op, int64_t C, int64_t inner, int per_channel, float mbits, int n_bits, int sign_bits, int x_mod16,
                   int y_type, fp8q_h16_route_info *info);

/*
 * The uniform (INT) quantizers on IEEE fp16 and bfloat16 tensors (csrc/fp8q_inth16.hip): fp8q_int_quantize_f32,
 * fp8q_int_range_quantize_f32 and fp8q_int_minmax_quantize_f32 with half x -- the argument lists of the _f32 twins, with
 * x_type / y_type (FP8Q_DT_*) behind x and y as in fp8q_quantize_h16.  Arithmetic contract:
 *   - every input element is widened to fp32 exactly, as the half-precision lane above does it: fp16 subnormals become
 *     normal numbers, bf16 is the upper half of an fp32 word, nothing is flushed;
 *   - from there the fp32 contract of the uniform quantizers applies unchanged, through the same code (the
 *     reciprocal-then-redo rule for x / scale included): the fp32 result is bit-identical to fp8q_int_quantize_f32 on the
 *     widened input.  Ranges (delta, zero_float, the sign byte, row min / max) are fp32;
 *   - y_type == FP8Q_DT_F32 stores that fp32 result; y_type == x_type rounds it ONCE to the storage type (round to nearest
 *     even, overflow to infinity: torch.Tensor.to(dtype)).  The fp32 value scale * (t - zp) exists before it is narrowed --
 *     the multiplication and the conversion are never fused into one rounding.  y may alias x then;
 *   - this is deliberately NOT the reference's arithmetic on a half tensor (with a 0-dim delta ATen rounds every op to the
 *     half type): it is the contract of the half-precision lane -- widen, compute in fp32, round once.
 * x (and a half y) need only their natural 2-byte alignment, an fp32 y 4 bytes; views at any element offset, y need not
 * share x's phase against the 16-byte grid; rows of any length (rows shorter than 8 elements and odd row lengths included).
 * Errors, all reported before any launch: FP8Q_EINVAL for null pointers, an x_type that is not a half type, a y_type that
 * is neither FP8Q_DT_F32 nor x_type, n_delta / n_range not in {1, C}, EMPTY tensors (C or inner <= 0), misaligned x / y and
 * the size limits of the _f32 twins (per-channel rows beyond 2^31 - 1 elements, more than 2^32 - 1 chunks of 4096 elements);
 * FP8Q_EUNSUPPORTED for n_bits outside [2, 16]; fp8q_int_minmax_quantize_h16: FP8Q_EWORKSPACE as fp8q_minmax_h16.
 *   fp8q_int_quantize_h16         fixed ranges: one launch.  HBM traffic: 4 B / element (half out), 6 B (fp32 out).
 *   fp8q_int_range_quantize_h16   int_set_range and the quantize in ONE launch (two for more than 2048 symmetric channels):
 *                                 delta / zero_float / signed_flag are bit-identical to fp8q_int_set_range_f32's.
 *   fp8q_int_minmax_quantize_h16  per-channel current_minmax: fp8q_minmax_h16's row scan (FP8Q_FOLD_CURRENT; ws / ws_bytes
 *                                 as there) writes row_min / row_max, then fp8q_int_range_quantize_h16 on them.  Two launches
 *                                 (three beyond 2048 symmetric channels), 2 B / element more.
 * Enqueue-only, no allocation.  FP8Q_VERSION is unchanged: the entries are additive.
 */
int fp8q_int_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *delta,
                          const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                          int symmetric, float eps, fp8q_stream_t stream);
int fp8q_int_range_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner,
                                const float *x_min, const float *x_max, int64_t n_range, float *delta, float *zero_float,
                                unsigned char *signed_flag, int n_bits, int symmetric, float eps, fp8q_stream_t stream);
int fp8q_int_minmax_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, float *row_min,
                                 float *row_max, float *delta, float *zero_float, unsigned char *signed_flag, int n_bits,
                                 int symmetric, float eps, void *ws, size_t ws_bytes, fp8q_stream_t stream);

/*
 * Storage codes of the half-precision lane (csrc/fp8q_codec_h16.hip): fp8q_encode_u8 / fp8q_decode_u8 and fp8q_int_encode /
 * fp8q_int_decode straight from and to IEEE fp16 and bfloat16 tensors -- the argument lists of those twins, with x_type /
 * y_type behind (x, codes) and (codes, y) as in fp8q_quantize_h16.  x_type / y_type is FP8Q_DT_F16 or FP8Q_DT_BF16; float32
 * values stay with the existing entry points.  Arithmetic contract:
 *   - every half input is widened to fp32 exactly, as the half-precision lane above does it: fp16 subnormals become normal
 *     numbers, bf16 is the upper half of an fp32 word, nothing is flushed.  From there the fp32 code runs unchanged, through
 *     the same device functions (the channel constants and scale tables, the encode assembly, the INT chain with its
 *     reciprocal-then-redo rule);
 *   - fp8q_encode_h16(x) == fp8q_encode_u8(widen(x)) byte for byte: NaN inputs and degenerate channels (maxval 0, inf or NaN)
 *     encode as 0; formats with n_bits > 8 or no exponent bit return FP8Q_EUNSUPPORTED;
 *   - fp8q_decode_h16(codes, y_type) takes the fp32 value of fp8q_decode_u8 and rounds it ONCE to y_type (round to nearest
 *     even, overflow to infinity: torch.Tensor.to(dtype)).  The fp32 value exists before it is narrowed -- the multiplication
 *     and the conversion are never fused into one rounding;
 *   - fp8q_int_encode_h16(x) == fp8q_int_encode(widen(x)): one byte for n_bits <= 8, two bytes (little endian) for 9..16, the
 *     same NaN and sign rules;
 *   - fp8q_int_decode_h16 takes fp8q_int_decode's fp32 value and rounds it once to y_type, in the same way.
 * Consequences: fp8q_decode_h16(fp8q_encode_h16(x), T) == fp8q_quantize_h16(x, y_type = T) bit for bit wherever the fp32
 * round trip equals K1 (the geometric-scale condition stated at fp8q_decode_u8: all weight-sized ranges); for INT,
 * fp8q_int_decode_h16(fp8q_int_encode_h16(x), T) == fp8q_int_quantize_h16(x, y_type = T) wherever x is not NaN.
 * Pointers need only natural alignment (2 bytes for halves and 2-byte INT codes, 1 byte for 1-byte codes); views at any
 * element offset, the codes need not share x's phase against the 16-byte grid; rows of any length (rows shorter than 8
 * elements and odd row lengths included).
 * Errors, all reported before any launch: FP8Q_EINVAL for null pointers, EMPTY tensors (C or inner <= 0), n_maxval / n_delta
 * not in {1, C}, a type that is not a half type, an odd address of a 2-byte element (2-byte INT codes included) and the size
 * limits of the twins (FP8: those of fp8q_quantize_h16; INT: those of fp8q_int_encode); FP8Q_EUNSUPPORTED as above, and for
 * INT n_bits outside [2, 16].
 * Each is ONE launch: enqueue-only, no allocation, no workspace.  HBM traffic: 3 B / element each way, 4 B with 2-byte INT
 * codes.  FP8Q_VERSION is unchanged: the entries are additive.
 */
int fp8q_encode_h16(const void *x, uint8_t *codes, int x_type, int64_t C, int64_t inner, const float *maxval,
                    int64_t n_maxval, float mbits, int n_bits, int sign_bits, fp8q_stream_t stream);
int fp8q_decode_h16(const uint8_t *codes, void *y, int y_type, int64_t C, int64_t inner, const float *maxval,
                    int64_t n_maxval, float mbits, int n_bits, int sign_bits, fp8q_stream_t stream);
int fp8q_int_encode_h16(const void *x, void *codes, int x_type, int64_t C, int64_t inner, const float *delta,
                        const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                        int symmetric, float eps, fp8q_stream_t stream);
int fp8q_int_decode_h16(const void *codes, void *y, int y_type, int64_t C, int64_t inner, const float *delta,
                        const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                        int symmetric, float eps, fp8q_stream_t stream);

/* ---- backward of the FP quantizer (csrc/fp8q_grad.hip) --------------------------------------------------------------------
 * The gradient of quantize_to_fp8_ste_MM (fp8_quantizer.py:105-133) with respect to x, maxval and the mantissa width, in
 * ONE streaming pass over x and the upstream gradient g (contiguous fp32 viewed as [C, inner], the layout rules of
 * fp8q_quantize_f32: n_maxval == 1 treats the tensor as one row).  With lo = -maxval (signed) or 0 (unsigned):
 *   gx[i]      = g[i] * m,  m = 1 strictly inside (lo, maxval), 0.5 exactly on a bound, 0 outside (a NaN x gives 0).  Exact.
 *   gmaxval[c] = sum over the row of g * w,  w = (y - xc) / maxval + [x > maxval] + 0.5 [x == maxval]
 *                                                - [x < lo] - 0.5 [x == lo]     (the last two terms: signed formats only)
 *   gmbits[0]  = ln2 (-1 - bias'(M)) * sum over everything of g * (y - xc),  bias'(M) = -ln2 2^E + 2^-M / (2 - 2^-M),
 *                M = clamp(rint(mbits), 1, n_bits - sign_bits); zero when rint(mbits) lies outside the clamp.
 * y is the forward's result, recomputed per element with the forward's own code (bit-identical to fp8q_quantize_f32), so
 * the caller keeps no y between forward and backward; xc = min(max(x, lo), maxval).  Each term is formed in fp32 in the order
 * written above, the sums are accumulated in fp64 in a fixed order (no floating-point atomics): two calls on the same buffers
 * give the same bits.  Any of gx, gmaxval [n_maxval], gmbits [1] may be NULL (not all three).
 * mbits_dev != NULL: the width is read from that device scalar (as fp8q_quantize_dm_f32), `mbits` is ignored, and the
 * rounding, the clamp test and the factor of gmbits are evaluated on the device: no host read of the width.
 * ws: 8-byte aligned, at least fp8q_quantize_bwd_workspace_bytes(C, inner, n_maxval) bytes, needed when gmaxval or gmbits is
 * requested (per-block partial sums; a second small launch adds them up).  The workspace rule of this library holds: zero
 * before the first use, left zero by every call.
 * HBM traffic: 12 B / element (x, g, gx), 8 B / element without gx.  Pointers need 4-byte alignment only.
 * Errors, all reported before any launch: FP8Q_EINVAL for null x / g / maxval, empty shapes (C or inner <= 0), n_maxval not
 * in {1, C}, sign_bits not in {0, 1}, misaligned fp32 pointers, gx == gmaxval == gmbits == NULL; FP8Q_EUNSUPPORTED for the
 * formats the forward refuses (more than 7 exponent bits); FP8Q_EWORKSPACE for a missing, misaligned or too small workspace.
 * Enqueue-only, no allocation.  FP8Q_VERSION is unchanged: the entries are additive.
 */
int fp8q_quantize_bwd_f32(const float *x, const float *g, float *gx, int64_t C, int64_t inner, const float *maxval,
                          int64_t n_maxval, float mbits, const float *mbits_dev, int n_bits, int sign_bits, float *gmaxval,
                          float *gmbits, void *ws, size_t ws_bytes, fp8q_stream_t stream);
size_t fp8q_quantize_bwd_workspace_bytes(int64_t C, int64_t inner, int64_t n_maxval);

/* ---- backward of the uniform (INT) quantizers (csrc/fp8q_intgrad.hip) -------------------------------------------------------
 * The gradient of fp8q_int_quantize_f32 (uniform_quantizers.py:108-164, linear scale domain, round_ste) with respect to x,
 * delta and zero_float, in ONE streaming pass over x and the upstream gradient g (contiguous fp32 viewed as [C, inner];
 * n_delta == 1 treats the whole tensor as one row, n_delta == C gives one sum per row).  The forward, fp32 throughout:
 *   scale = max(delta, eps);  zp = clamp(rint(zero_float), lo, hi) (0 when symmetric);  [lo, hi] as fp8q_int_quantize_f32,
 *   the symmetric sign read from the device byte signed_flag;  t = fl32(x / scale), the IEEE quotient;  u = rint(t) + zp;
 *   v = clamp(u, lo, hi);  y = scale * (v - zp).
 * With m = 1.0f when lo <= u <= hi (bounds inclusive, as ATen's clamp backward), else 0.0f (a NaN u gives 0):
 *   gx[i]          = g[i] * m.  Exact (the autograd chain forms (g * scale) * m / scale: the same value up to 1 ULP).
 *   gdelta[c]      = [delta_c >= eps] * sum over the row of g * w,  w = (v - zp) - fl32(m * t), each term formed in fp32 in
 *                    that order.  The product m * t is deliberate: x = +-inf gives 0 * inf = NaN, a NaN x is NaN as well,
 *                    and such a row gets a NaN gradient -- as the chain's 0 * ((x / scale) / scale) does.
 *   gzero_float[c] = -[lo <= rint(zero_float_c) <= hi] * sum over the row of (1 - m) * fl32(g * scale)   (asymmetric only)
 * A false mask gives exactly 0.  The sums are accumulated in fp64 in a fixed order (no floating-point atomics): two calls on
 * the same buffers give the same bits.
 * grad_scale_elems > 0 (LSQ's gradient scaling, calculate_grad_scale, uniform_quantizers.py:166-173): both sums, after they
 * are rounded to fp32, are multiplied by gs = (float)(1 / sqrt((double)hi * (double)grad_scale_elems)), hi the positive end
 * of the integer range -- taken from signed_flag when symmetric, so there is no host read.  The caller passes numel / C per
 * channel and numel per tensor.  0: no scaling.
 * Any of gx, gdelta [n_delta], gzero_float [n_delta] may be NULL (not all three); gzero_float with symmetric is
 * FP8Q_EINVAL.  zero_float may be NULL when symmetric, signed_flag when not.
 * ws: 8-byte aligned, at least fp8q_int_quantize_bwd_workspace_bytes(C, inner, n_delta) bytes, needed when gdelta or
 * gzero_float is requested (per-block partial sums; a second small launch adds them up and applies the masks and gs).  The
 * workspace rule of this library holds: zero before the first use, left zero by every call.
 * HBM traffic: 12 B / element (x, g, gx), 8 B / element without gx.  Pointers need 4-byte alignment only.
 * Errors, all reported before any launch: FP8Q_EINVAL for null or misaligned pointers, empty shapes (C or inner <= 0),
 * n_delta not in {1, C}, a negative grad_scale_elems, gx == gdelta == gzero_float == NULL; FP8Q_EUNSUPPORTED for n_bits
 * outside [2, 16]; FP8Q_EWORKSPACE for a missing, misaligned or too small workspace.
 * Enqueue-only, no allocation.  FP8Q_VERSION is unchanged: the entries are additive.
 */
size_t fp8q_int_quantize_bwd_workspace_bytes(int64_t C, int64_t inner, int64_t n_delta);
int fp8q_int_quantize_bwd_f32(const float *x, const float *g, float *gx, int64_t C, int64_t inner, const float *delta,
                              const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits,
                              int symmetric, float eps, int64_t grad_scale_elems, float *gdelta, float *gzero_float, void *ws,
                              size_t ws_bytes, fp8q_stream_t stream);

/*
 * Percentile ranges (CurrentMinMaxEstimator(percentile=p), range_estimators.py:61-70: np.percentile(x, (p, 100 - p))):
 * lo[c], hi[c] of every row of a contiguous [C, inner] float32 tensor by EXACT selection -- a radix select over integer
 * keys, no sort, no floating-point sums (csrc/fp8q_select.hip).  Arithmetic contract, for one row of n = inner elements:
 *   1. Ordering: by the monotone unsigned key of the bit pattern (non-negative numbers set the sign bit, negative numbers
 *      invert all bits): -inf < ... < -0.0 < +0.0 < ... < +inf, the -0.0 < +0.0 rule of the min/max folds.  s[0 .. n-1] is
 *      the row in that order.
 *   2. Ranks, on the host in double (they depend on the shape only: nothing is read back from the device): the quantiles are
 *      q_lo = pct / 100.0 and q_hi = (100.0 - pct) / 100.0, the reference's operands; for each,
 *      pos = q * (double)(n - 1), k = min(max((int64)floor(pos), 0), n - 1), k1 = min(k + 1, n - 1), t = pos - (double)k.
 *   3. Interpolation, in double: a = s[k], b = s[k1], d = (double)(float)(b - a) -- the difference is rounded to float32
 *      first, as numpy does with float32 data; t < 0.5: v = (double)a + d * t, otherwise v = (double)b - d * (1.0 - t);
 *      the result is (float)v, one rounding.  +-inf follow the formula (inf - inf gives NaN, as in numpy).
 *   4. NaN: a row that holds a NaN anywhere gives NaN for both lo and hi, as np.percentile does; other rows are unaffected.
 * The result is a function of the row's multiset of values only: deterministic, independent of the launch geometry.
 * Rows up to fp8q_percentile_resident_max_inner() elements are selected from an LDS copy in one launch and need no
 * workspace (ws may be NULL with ws_bytes == 0).  Longer rows take three counting passes over x (11 + 11 + 10 key bits) with
 * a tiny launch after each -- six launches and one memset node, none waits on another -- and need
 * fp8q_percentile_workspace_bytes(C, inner) bytes at `ws`, 8-byte aligned; the workspace need not be initialised (the
 * call clears what it counts into) and holds nothing between calls.
 * Errors, all reported before any HIP call: FP8Q_EINVAL for null pointers, C < 1 or inner < 1, pct NaN or outside
 * [0, 100], pointers that are not 4-byte aligned, a missing, misaligned or too small workspace; FP8Q_EUNSUPPORTED for
 * streaming rows of 2^32 elements or more, or more than 2^30 such rows.
 * Enqueue-only, no allocation.  FP8Q_VERSION is unchanged: the entries are additive.
 */
int64_t fp8q_percentile_resident_max_inner(void);
size_t fp8q_percentile_workspace_bytes(int64_t C, int64_t inner);
int fp8q_percentile_f32(const float *x, int64_t C, int64_t inner, double pct, float *lo, float *hi, void *ws, size_t ws_bytes,
                        fp8q_stream_t stream);

/* ---- hardware FP8: the OCP encodings E4M3FN and E5M2 (csrc/fp8q_ocp.hip) ---------------------------------------------------
 * Every other lane of this library computes the reference's emulated formats (a real-valued exponent bias, the top exponent
 * code an ordinary binade); their storage codes cannot be fed to gfx950's matrix cores or read as torch.float8_e4m3fn /
 * torch.float8_e5m2: the byte of a channel's largest element is all ones below the sign, which E4M3FN reads as NaN.  These
 * entries produce and read the OCP bytes themselves, with the chip's conversion instructions.
 * Arithmetic contract.  fmt is FP8Q_OCP_E4M3FN (fmax = 448) or FP8Q_OCP_E5M2 (fmax = 57344); maxval holds 1 or C entries:
 *   scale = max(maxval, eps) / fmax          float32, IEEE division, torch.max: a NaN maxval gives a NaN scale
 *   q     = clamp(x / scale, -fmax, fmax)    float32 IEEE division, then torch.clamp: NaN passes, +-inf saturate to +-fmax
 *   code  = RNE(q) as an OCP byte            subnormals as OCP defines them, -0 -> 0x80, every NaN -> 0x7F in both formats
 *                                            (the sign of a NaN is not kept).  Overflow codes -- E4M3FN's NaN, E5M2's
 *                                            infinity -- are never produced from finite or infinite x: the clamp comes first,
 *                                            so the conversion instruction's own overflow behaviour is never relied on.
 *   decode(code) = value(code) * scale       ONE float32 multiplication; a half output rounds that product once (round to
 *                                            nearest even, as torch.Tensor.to(dtype)).  A NaN code is not multiplied: it
 *                                            decodes to the NaN torch's widening gives it (sign, quiet bit, the code's
 *                                            mantissa field left aligned: 0x7FF00000 for E4M3FN 0x7F).
 *   quantize(x) = decode(encode(x))          bit for bit, in one pass.
 * The oracle is torch's CPU cast: torch.clamp(x / scale, -fmax, fmax).to(torch.float8_e4m3fn) and c.float() * scale.  The
 * kernels multiply by 1 / scale and redo the division wherever the product lies within the reciprocal's error of a rounding
 * boundary (the bound is derived at the top of fp8q_ocp.hip), so the codes are those of the division.
 * Half inputs (x_type = FP8Q_DT_F16 / FP8Q_DT_BF16) are widened exactly; fp8q_ocp_quantize_h16's y_type is FP8Q_DT_F32 or
 * x_type, as in fp8q_quantize_h16.  scale_out (encode, may be NULL) receives the 1 or C scales, each written by the block
 * in whose chunk the row starts; fp8q_ocp_scale_f32 computes the same n values from a range alone.  fp8q_ocp_decode_* take
 * those scales, not the range.  codes with scale as a per-row [C, 1] or per-tensor [1] factor are the operands a scaled
 * FP8 matrix multiplication takes; nothing here performs one.
 * Per tensor (n_maxval == 1) and per channel (n_maxval == C), rows of any length.  fp32 pointers need 4-byte, half pointers
 * 2-byte alignment (FP8Q_EINVAL); 16-byte aligned x / y / codes take the vector route (a lane converts 16 consecutive
 * elements and stores 16 codes as one word), anything else goes element by element with the same results.
 * Errors, all reported before the launch: FP8Q_EINVAL for null pointers, empty shapes (C or inner <= 0), n_maxval / n_scale
 * not in {1, C}, misaligned pointers, a type that is not a half type (y_type: nor FP8Q_DT_F32); FP8Q_EUNSUPPORTED for any
 * other fmt.  One launch per call, enqueue-only, no workspace.  FP8Q_VERSION is unchanged: the entries are additive.
 */
#define FP8Q_OCP_E4M3FN 0
#define FP8Q_OCP_E5M2 1
int fp8q_ocp_encode_f32(const float *x, uint8_t *codes, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                        int fmt, float eps, float *scale_out, fp8q_stream_t stream);
int fp8q_ocp_encode_h16(const void *x, uint8_t *codes, int x_type, int64_t C, int64_t inner, const float *maxval,
                        int64_t n_maxval, int fmt, float eps, float *scale_out, fp8q_stream_t stream);
int fp8q_ocp_decode_f32(const uint8_t *codes, float *y, int64_t C, int64_t inner, const float *scale, int64_t n_scale, int fmt,
                        fp8q_stream_t stream);
int fp8q_ocp_decode_h16(const uint8_t *codes, void *y, int y_type, int64_t C, int64_t inner, const float *scale,
                        int64_t n_scale, int fmt, fp8q_stream_t stream);
int fp8q_ocp_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval, int fmt,
                          float eps, fp8q_stream_t stream);
int fp8q_ocp_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *maxval,
                          int64_t n_maxval, int fmt, float eps, fp8q_stream_t stream);
int fp8q_ocp_scale_f32(const float *maxval, int64_t n, int fmt, float eps, float *scale, fp8q_stream_t stream);

/* ---- hardware FP8 under one float32 scale per TILE: 1x128, 128x1 and 128x128 (csrc/fp8q_ocp_block.hip) ----------------------
 * The operand form of block-scaled FP8 matrix multiplications: E4M3FN / E5M2 elements, a float32 scale per tile -- 1x128 along
 * the reduction dimension for activations, 128x128 for weights, 128x1 for the operand of a product that reduces over dim 0
 * (dW = dy^T . x).  The range of a tile is found inside the pass: there is nothing to calibrate, and x is read once.
 * x is [R, K], K contiguous, float32 or a half type (widened exactly).  fmt is FP8Q_OCP_E4M3FN or FP8Q_OCP_E5M2.  The tile
 * (tile_r, tile_k) is (1, 128), (128, 1) or (128, 128); anything else is FP8Q_EUNSUPPORTED.  Tile (i, j) covers the rows
 * [tile_r i, min(tile_r i + tile_r, R)) and the columns [tile_k j, min(tile_k j + tile_k, K)): edge tiles are short, and no
 * tile wraps.
 *   amax = torch.amax(|x|) over the tile     a NaN anywhere in the tile gives NaN, an infinity gives inf
 *   codes and scale of the tile              byte for byte what the per-tensor call above gives on that tile alone,
 *                                            fp8q_ocp_encode_* on x[tile] with maxval = amax and the same eps, and its scale_out:
 *                                            scale = max(amax, eps) / fmax, q = clamp(x / scale, -fmax, fmax), code = RNE(q),
 *                                            every NaN stored as 0x7F
 *   decode = value(code) * scale             one float32 multiplication; a NaN code is not multiplied; a half output rounds
 *                                            that product once
 *   quantize = decode(encode)                bit for bit, in one launch, the scales never leaving the chip
 * What follows from these rules (nothing below is a special case of the code):
 *   - an all-zero tile has scale = eps / fmax and zero codes;
 *   - a tile with a NaN has a NaN scale and every code 0x7F;
 *   - a tile with an infinity has scale = inf: its finite elements encode to +-0, its infinities to 0x7F (inf / inf), and
 *     every element of it decodes to NaN (0 * inf).
 * Layout: codes is [R, K] bytes in x's own layout for all three tiles (nothing is transposed); scales is float32
 * [ceil(R / tile_r), ceil(K / tile_k)], row-major, in no library's swizzle.  Power-of-two (UE8M0) tile scales are the MX
 * lane's business, not this one's.
 * Routes.  fp8q_ocpb_route is host arithmetic only: it returns the kernel (FP8Q_OCPB_*) that encode and quantize reach for
 * a shape, or the error they would report; aligned16: x and codes / y start on 16 bytes.
 *   FP8Q_OCPB_ROWS   (1, 128) with K % 128 == 0 and aligned16: a flat run of whole tiles, half a wave per tile
 *   FP8Q_OCPB_PANEL  (128, 1) and (128, 128) with K % 4 == 0 and aligned16: a 128 x 128 panel per workgroup, held in registers
 *                    (x is read once); ragged R and K are its own edge panels
 *   FP8Q_OCPB_PLAIN  anything else: one wave per tile, element by element, the same bytes
 * Decode takes the codes by dwords where K % 4 == 0 and codes / y start on 16 bytes, element by element otherwise.
 * Errors, all reported before the launch: FP8Q_EINVAL for null pointers, R or K <= 0 (or an R * K beyond int64, a grid beyond
 * INT32_MAX), a value pointer off its element's alignment, scales off 4 bytes, a type that is not a half type on an _h16
 * entry (y_type: nor FP8Q_DT_F32) or two different half types; FP8Q_EUNSUPPORTED for any other fmt or tile.  One launch per
 * call, enqueue-only, no workspace.  FP8Q_VERSION is unchanged: the entries are additive.
 */
#define FP8Q_OCPB_ROWS 0
#define FP8Q_OCPB_PANEL 1
#define FP8Q_OCPB_PLAIN 2
int fp8q_ocpb_route(int64_t R, int64_t K, int tile_r, int tile_k, int x_type, int aligned16);
int fp8q_ocpb_encode_f32(const float *x, uint8_t *codes, float *scales, int64_t R, int64_t K, int tile_r, int tile_k, int fmt,
                         float eps, fp8q_stream_t stream);
int fp8q_ocpb_encode_h16(const void *x, uint8_t *codes, float *scales, int x_type, int64_t R, int64_t K, int tile_r, int tile_k,
                         int fmt, float eps, fp8q_stream_t stream);
int fp8q_ocpb_decode_f32(const uint8_t *codes, const float *scales, float *y, int64_t R, int64_t K, int tile_r, int tile_k,
                         int fmt, fp8q_stream_t stream);
int fp8q_ocpb_decode_h16(const uint8_t *codes, const float *scales, void *y, int y_type, int64_t R, int64_t K, int tile_r,
                         int tile_k, int fmt, fp8q_stream_t stream);
int fp8q_ocpb_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int tile_r, int tile_k, int fmt, float eps,
                           fp8q_stream_t stream);
int fp8q_ocpb_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int tile_r, int tile_k,
                           int fmt, float eps, fp8q_stream_t stream);

/* ---- the same operands TRANSPOSED: those of x^T, made from x as it lies (csrc/fp8q_ocp_block_t.hip) -------------------------
 * A block-scaled FP8 product takes both operands with the reduction dimension contiguous.  The backward products reduce over
 * dim 0 of x -- dx = dy . W over W's rows, dW = dy^T . x over the tokens -- so they need the 1x128 operands of x^T and dy^T
 * and the 128x128 operand of W^T, laid out [K, R].  x is [R, K], K contiguous, float32 or a half type (widened exactly).
 * Contract, by reference: the transposed operands of x are, byte for byte, the operands of the contiguous [K, R] tensor x^T
 * under the tile-scaled contract above, same fmt, tile and eps.  codes_t is [K, R] bytes; scales_t is float32, row-major,
 * [K, ceil(R / 128)] for (1, 128) -- column c of x is cut into the tiles of rows [128 i, min(128 i + 128, R)) -- and
 * [ceil(K / 128), ceil(R / 128)] for (128, 128).  fp8q_ocpb_decode_* reads them as the [K, R] operands they are (it gives the
 * values of x^T); there is no transposing decode and no transposed quantize: fake-quantization in x's own layout under the
 * transposed (1, 128) tiles is fp8q_ocpb_quantize_* with the tile (128, 1).
 *   fp8q_ocpbt_encode_*       writes codes_t and scales_t
 *   fp8q_ocpbt_encode_both_*  writes codes / scales, equal to fp8q_ocpb_encode_*'s, and codes_t / scales_t, equal to
 *                             fp8q_ocpbt_encode_*'s, from one read of x.  (1, 128): two quantizations, row tiles and column
 *                             tiles have their own scales.  (128, 128): one quantization stored twice, codes_t and scales_t
 *                             are the transposes of codes and scales
 * The tile is (1, 128) or (128, 128).  (128, 1) is FP8Q_EUNSUPPORTED here, like every other tile: its result would be x's
 * 1x128 quantization with transposed codes, the operand of no product.  The special tiles (all zero, a NaN, an infinity)
 * follow from the contract above, as there.
 * fp8q_ocpbt_route is host arithmetic only and is the launchers' own rule: aligned16 says whether EVERY pointer of the call
 * starts on 16 bytes.
 *   FP8Q_OCPBT_PANEL  K % 4 == 0 and aligned16: a 128 x 128 panel per workgroup, held in registers (x is read once), the
 *                     transposed codes turned in LDS and stored along R in words of code_store_bytes
 *   FP8Q_OCPBT_PLAIN  anything else: one wave per tile, element by element, the same bytes (encode_both at (1, 128) reads x
 *                     twice there)
 * Errors, all reported before the launch: FP8Q_EINVAL for null pointers (the route: a null info), R or K <= 0 (or an R * K
 * beyond int64, a grid beyond INT32_MAX), a value pointer off its element's alignment, scales or scales_t off 4 bytes, a type
 * that is not a half type on an _h16 entry; FP8Q_EUNSUPPORTED for any other fmt or tile.  One launch per call, enqueue-only,
 * nothing read back, no workspace.
 * Names: these entries are fp8q_ocpbt_*: the set of fp8q_ocpb_* entries is the lane's seven.  FP8Q_VERSION is unchanged: the
 * entries are additive.
 */
#define FP8Q_OCPBT_PANEL 0
#define FP8Q_OCPBT_PLAIN 1
typedef struct fp8q_ocpbt_route_info {
    int kernel;             /* FP8Q_OCPBT_PANEL or FP8Q_OCPBT_PLAIN */
    int code_store_bytes;   /* bytes per store of transposed codes on the panel route: 16 where R % 16 == 0, 4 where R % 4 == 0,
                               else 1; 1 on the plain route */
    int nontemporal;        /* the panel kernel's nontemporal variant (R * K * 4 bytes from 64 MiB) */
    int reserved;
} fp8q_ocpbt_route_info;
int fp8q_ocpbt_route(int64_t R, int64_t K, int tile_r, int tile_k, int x_type, int aligned16, fp8q_ocpbt_route_info *info);
int fp8q_ocpbt_encode_f32(const float *x, uint8_t *codes_t, float *scales_t, int64_t R, int64_t K, int tile_r, int tile_k,
                          int fmt, float eps, fp8q_stream_t stream);
int fp8q_ocpbt_encode_h16(const void *x, uint8_t *codes_t, float *scales_t, int x_type, int64_t R, int64_t K, int tile_r,
                          int tile_k, int fmt, float eps, fp8q_stream_t stream);
int fp8q_ocpbt_encode_both_f32(const float *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int64_t R,
                               int64_t K, int tile_r, int tile_k, int fmt, float eps, fp8q_stream_t stream);
int fp8q_ocpbt_encode_both_h16(const void *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int x_type,
                               int64_t R, int64_t K, int tile_r, int tile_k, int fmt, float eps, fp8q_stream_t stream);

/* ---- microscaling (MX): blocks of 32 under an E8M0 scale byte, elements in E4M3FN / E5M2 / E2M3 / E3M2 / E2M1 ----------------
 * (csrc/fp8q_mx.hip)  The operand forms of gfx950's scaled matrix instructions (v_mfma_scale_f32_*_f8f6f4), carried by
 * torch.float8_e8m0fnu and torch.float4_e2m1fn_x2 (the 6-bit formats have no torch dtype: plain bytes).  These entries make, read and fake-quantize such operands; nothing here performs the multiplication,
 * and the scale bytes are in plain [R, ceil(K / 32)] order, not in any library's pre-swizzled layout.
 * Arithmetic contract.  The tensor is [R, K], K contiguous.  Row r is cut into the blocks [32j, min(32j + 32, K)): the last
 * block of a row may be short, and no block crosses a row.
 *   fmt              emax    fmax    mantissa field of fmax (man_fmax)
 *   FP8Q_MX_E4M3FN     8      448    0x600000
 *   FP8Q_MX_E5M2      15    57344    0x600000
 *   FP8Q_MX_E2M1       2        6    0x400000
 *   FP8Q_MX_E2M3       2      7.5    0x700000        s1 e2 m3, bias 1
 *   FP8Q_MX_E3M2       4       28    0x600000        s1 e3 m2, bias 3
 * The scale byte of a block, in integer arithmetic only:
 *   m    = the largest of the block's bits(|x|), compared as unsigned integers (NaN and inf patterns are the largest)
 *   E    = m >> 23, man = m & 0x7fffff
 *   code = max(E - emax + bump, 0);  0xFF when E == 255 (a NaN or an infinity anywhere in the block); a zero or
 *          subnormal-only block gives 0
 *   bump = 0 for FP8Q_MX_FLOOR, the OCP MX v1.0 rule X = 2^(floor(log2 amax) - emax): elements above fmax * X saturate;
 *          (man > man_fmax) for FP8Q_MX_CEIL: the smallest power of two under which no element saturates
 *   X    = 2^(code - 127) as float32: code 0 is the subnormal 0x00400000, 0xFF is NaN
 * Elements:
 *   q    = clamp(x * 2^(127 - code), -fmax, fmax)   ONE float32 multiplication by an exactly representable power of two.  It
 *          is exact except where it lands in float32's subnormal range, which is far below every format's smallest
 *          midpoint: those elements are a zero of x's sign either way
 *   elem = RNE(q) in the element format, subnormals included; -0 keeps its sign (0x80 in FP8, 0x20 in FP6, 0x8 in FP4)
 *   a 0xFF block stores 0x7F (FP8) / 0x0 (FP6, FP4) in every element
 *   E2M1: the codes 0..7 are the values {0, .5, 1, 1.5, 2, 3, 4, 6}, the sign is bit 3, a tie goes to the even code; two
 *   elements share a byte, the even-indexed one in the low nibble, so codes holds R * K / 2 bytes and K must be even
 *   E2M3, E3M2 (FP6): the magnitude code c is the low 5 bits and the sign is bit 5; there is no NaN and no infinity among
 *   the 64 codes; a tie goes to the even code
 *     E2M3: e = c >> 3, m = c & 7; the value is m * 0.125 for e == 0, else (1 + m / 8) * 2^(e - 1)
 *     E3M2: e = c >> 2, m = c & 3; the value is m * 0.0625 for e == 0, else (1 + m / 4) * 2^(e - 3)
 *   The FP6 codes of a row are one little-endian bit string, element i in bits [6i, 6i + 6): four elements are three bytes,
 *   b0 = e0 | e1 << 6, b1 = e1 >> 2 | e2 << 4, b2 = e2 >> 4 | e3 << 2.  K must be a multiple of 4 (the counterpart of E2M1's
 *   even K): then no byte is shared between rows and every block, ragged or not, starts on a byte.  codes holds R * 3K / 4
 *   bytes; a full block is 24 bytes, the 6-VGPR operand of the matrix instruction
 * decode(elem) = value(elem) * X, ONE float32 multiplication; subnormal products are kept; every element of a 0xFF block
 * decodes to NaN, as does a NaN element code; a half output rounds the float32 product once (round to nearest even).
 * quantize(x) = decode(encode(x)) bit for bit, in one launch.  Half inputs are widened exactly; fp8q_mx_quantize_h16's y_type
 * is FP8Q_DT_F32 or x_type.
 * scales holds R * ceil(K / 32) bytes in row-major order; encode writes it, decode reads it, quantize keeps it in registers.
 * K % 32 == 0 with x / y / codes 16-byte aligned takes the vector route (the range is found in the wave, every element is
 * read once); anything else goes block by block, one lane each, with the same results.
 * Errors, all reported before the launch: FP8Q_EINVAL for null pointers, empty shapes (R or K <= 0), an fp32 pointer off its
 * 4-byte / a half pointer off its 2-byte alignment, an odd K with FP8Q_MX_E2M1, a K that is no multiple of 4 with
 * FP8Q_MX_E2M3 / FP8Q_MX_E3M2, an unknown rounding, a type that is not a half type (y_type: nor FP8Q_DT_F32) or two different
 * half types; FP8Q_EUNSUPPORTED for any other fmt -- the id 3 included, which stays unassigned.  One launch per call,
 * enqueue-only, no workspace.  FP8Q_VERSION is unchanged: the entries, and the two FP6 ids they take, are additive.
 */
#define FP8Q_MX_E4M3FN 0
#define FP8Q_MX_E5M2 1
#define FP8Q_MX_E2M1 2
#define FP8Q_MX_E2M3 4
#define FP8Q_MX_E3M2 5
#define FP8Q_MX_FLOOR 0
#define FP8Q_MX_CEIL 1
int fp8q_mx_encode_f32(const float *x, uint8_t *codes, uint8_t *scales, int64_t R, int64_t K, int fmt, int rounding,
                       fp8q_stream_t stream);
int fp8q_mx_encode_h16(const void *x, uint8_t *codes, uint8_t *scales, int x_type, int64_t R, int64_t K, int fmt,
                       int rounding, fp8q_stream_t stream);
int fp8q_mx_decode_f32(const uint8_t *codes, const uint8_t *scales, float *y, int64_t R, int64_t K, int fmt,
                       fp8q_stream_t stream);
int fp8q_mx_decode_h16(const uint8_t *codes, const uint8_t *scales, void *y, int y_type, int64_t R, int64_t K, int fmt,
                       fp8q_stream_t stream);
int fp8q_mx_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, fp8q_stream_t stream);
int fp8q_mx_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                         fp8q_stream_t stream);

/* ---- microscaling with the blocks along dim 0: the operands of the transpose, made from x as it lies -----------------------
 * (csrc/fp8q_mx_t.hip)  A product that reduces over dim 0 of x -- dx = dy . W over W's rows, dW = dy^T . x over the tokens --
 * needs x's MX blocks along dim 0, and those are not a permutation of the row-wise ones.  x is [R, K], K contiguous, float32
 * or a half type (widened exactly).
 * Contract, by reference: the transposed operands of x are, byte for byte, the operands of the contiguous [K, R] tensor x^T
 * under the MX contract above (the same scale rule, the 0xFF block, element arithmetic and packing; fmt and rounding as
 * there).  So column c of x is cut into the blocks of rows [32j, min(32j + 32, R)); codes_t is [K, R] bytes for FP8,
 * [K, R / 2] for E2M1 (rows 2i and 2i + 1 of a column share a byte) and [K, 3R / 4] for FP6 (four consecutive rows of a column
 * are three bytes); scales_t is [K, ceil(R / 32)].  fp8q_mx_decode_* reads them as the [K, R] operands they are; there is no
 * transposing decode.
 *   fp8q_mxt_encode_*       writes codes_t and scales_t
 *   fp8q_mxt_encode_both_*  writes codes / scales, equal to fp8q_mx_encode_*'s, and codes_t / scales_t, equal to
 *                           fp8q_mxt_encode_*'s, from one read of x
 *   fp8q_mxt_quantize_*     fake-quantize in x's own layout: y[r][c] = the decode of the transposed operands at [c][r]; the
 *                           type pairs are fp8q_mx_quantize_*'s
 * Divisibility: an encoder packs codes along R, so fp8q_mxt_encode_* needs an even R for FP8Q_MX_E2M1 and R % 4 == 0 for the
 * FP6 formats, and fp8q_mxt_encode_both_* needs the same of R and of K.  fp8q_mxt_quantize_* packs nothing and takes every R
 * and K.
 * Errors, all reported before the launch, as the MX entries report them: FP8Q_EINVAL for null pointers, R or K <= 0, a value
 * pointer off its element's alignment, an unknown rounding, the divisibility above, a wrong type or pair of types, a size
 * whose element count or grid overflows; FP8Q_EUNSUPPORTED for any other fmt, 3 included.
 * fp8q_mxt_route is host arithmetic only: it reports the kernel the three entries reach for a shape -- every launcher calls
 * it -- so that a test can assert the route before it trusts a shape.  aligned16: whether every pointer of the call is
 * 16-byte aligned.  The tile kernel (rows readable with 16-byte loads: K % 4 == 0 for float32, K % 8 == 0 for a half type;
 * aligned16) reads every element once and writes codes_t in runs of a tile's rows; anything else goes block by block, one
 * lane each, with the same results.  One launch per call, enqueue-only, no workspace.
 * Names: these entries are fp8q_mxt_*, not fp8q_mx_*_t: the set of fp8q_mx_* entries is the row-wise lane's six.
 * FP8Q_VERSION is unchanged: the entries are additive.
 */
#define FP8Q_MXT_TILE 0
#define FP8Q_MXT_GENERAL 1
typedef struct fp8q_mxt_route_info {
    int kernel;             /* FP8Q_MXT_TILE or FP8Q_MXT_GENERAL */
    int tile_rows;          /* rows of x under one workgroup of the tile kernel: a multiple of 32 */
    int tile_cols;          /* its columns: a multiple of 4 */
    int nontemporal;        /* the tile kernel's nontemporal variant (R * K * 4 bytes from 64 MiB) */
    int code_store_bytes;   /* bytes per store of transposed codes: 16 where a codes_t row is a multiple of 16 bytes, else 4
                               or 1 (the encoders on the tile kernel; 1 on the general route) */
    int reserved;
} fp8q_mxt_route_info;
int fp8q_mxt_route(int64_t R, int64_t K, int fmt, int x_type, int aligned16, fp8q_mxt_route_info *info);
int fp8q_mxt_encode_f32(const float *x, uint8_t *codes_t, uint8_t *scales_t, int64_t R, int64_t K, int fmt, int rounding,
                        fp8q_stream_t stream);
int fp8q_mxt_encode_h16(const void *x, uint8_t *codes_t, uint8_t *scales_t, int x_type, int64_t R, int64_t K, int fmt,
                        int rounding, fp8q_stream_t stream);
int fp8q_mxt_encode_both_f32(const float *x, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int64_t R,
                             int64_t K, int fmt, int rounding, fp8q_stream_t stream);
int fp8q_mxt_encode_both_h16(const void *x, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int x_type,
                             int64_t R, int64_t K, int fmt, int rounding, fp8q_stream_t stream);
int fp8q_mxt_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, fp8q_stream_t stream);
int fp8q_mxt_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                          fp8q_stream_t stream);

/* ---- microscaling with seeded stochastic rounding of the elements, every orientation ------------------------------------------
 * (csrc/fp8q_mxq.h, used by csrc/fp8q_mx.hip and csrc/fp8q_mx_t.hip)  Round to nearest even is biased on a gradient at 4 to 8
 * bits: whatever is smaller than half a grid step disappears, in every block, every step, in the same direction.  These ten
 * entries are the twins of the MX entries that convert elements, with `uint64_t seed, uint64_t offset` in front of `stream`.
 * Everything up to q is the MX contract above: the scale byte (either rule, the 0xFF block, code 0) and
 * q = clamp(x * 2^(127 - code), -fmax, fmax) are unchanged, and a 0xFF block stores what it stores there.  Only
 *   elem = RNE(q)   becomes   elem = RNE(SR(q, r))
 * where SR returns a float32 ON the element format's grid, so the conversion after it is exact.
 *
 * The draw.  Element i = offset + r * K + c mod 2^64 is the flat index in x AS IT LIES (the transposed entries index by the
 * position in x, not in x^T); offset must be a multiple of 8.  Element i takes 16 bits of one Philox4x32-10 call:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (g & 0xffffffff, g >> 32, 0, 0)          g = i >> 3
 *   w       = out[(i >> 1) & 3]
 *   r       = (w >> (16 * (i & 1))) & 0xffff
 * Philox4x32-10 is the standard one: multipliers 0xD2511F53 and 0xCD9E8D57, Weyl constants 0x9E3779B9 and 0xBB67AE85, ten
 * rounds.  Known answers (counter words, key words -> output words): all zero -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all
 * ffffffff -> 408f276d 41c83b0e a20bc7c6 6d5451fd; 243f6a88 85a308d3 13198a2e 03707344 with key a4093822 299f31d0 ->
 * d16cfe09 94fdcceb 5001e420 24126ea1.  An aligned group of four flat indices lies in one call (words 0, 1 or 2, 3).  The
 * draw belongs to the element, not to the kernel: the same (seed, offset) gives the same r for the same element in all ten
 * entries, so quantize == decode(encode), encode_both == (encode, encode_t), and a slice encoded with the offset of its first
 * element equals the slice of the whole.
 *
 * The rounding.  M mantissa bits and exponent bias B: E4M3FN 3, 7; E5M2 2, 15; E2M3 3, 1; E3M2 2, 3; E2M1 1, 1.
 * a = bits(|q|).
 *   normal range, |q| >= 2^(1 - B):  sh = 23 - M, f16 = (a >> (sh - 16)) & 0xffff, a' = (a >> sh) + ((f16 + r) >> 16); the
 *     magnitude is the float32 with bits a' << sh.  The carry runs into the exponent; fmax is a grid point (f16 = 0), so
 *     nothing passes it and E4M3FN never reaches 0x7F.
 *   format-subnormal range, |q| < 2^(1 - B), grid step 2^(1 - B - M):  u = (uint32) floor(|q| * 2^(16 + B + M - 1)), one
 *     float32 product, below 2^(M + 16); n = (u + r) >> 16; the magnitude is n * 2^(1 - B - M), n = 2^M being the smallest
 *     normal.
 *   The sign of q is kept, on a zero result too (the -0 codes).
 * So P(round away from zero) = floor(f * 2^16) / 2^16 with f the element's position between its two neighbours, grid points
 * never move, the result is always one of the two neighbours, and the bias toward zero is below 2^-16 of a step.  Half inputs
 * are widened exactly; half outputs of quantize round the float32 product once, as in the MX entries.
 *
 * Errors are the twin's, all reported before the launch; an offset that is no multiple of 8 is FP8Q_EINVAL.  Routes, launch
 * geometry and traffic are the twin's.  gfx950's own stochastic conversions (v_cvt_scalef32_sr_*) are not used, for the
 * reason the MX lane gives for the scaled conversions. */
int fp8q_mxsr_encode_f32(const float *x, uint8_t *codes, uint8_t *scales, int64_t R, int64_t K, int fmt, int rounding,
                         uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_mxsr_encode_h16(const void *x, uint8_t *codes, uint8_t *scales, int x_type, int64_t R, int64_t K, int fmt,
                         int rounding, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_mxsr_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, uint64_t seed,
                           uint64_t offset, fp8q_stream_t stream);
int fp8q_mxsr_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                           uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_mxsr_encode_t_f32(const float *x, uint8_t *codes_t, uint8_t *scales_t, int64_t R, int64_t K, int fmt, int rounding,
                           uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_mxsr_encode_t_h16(const void *x, uint8_t *codes_t, uint8_t *scales_t, int x_type, int64_t R, int64_t K, int fmt,
                           int rounding, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_mxsr_encode_both_f32(const float *x, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int64_t R,
                              int64_t K, int fmt, int rounding, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_mxsr_encode_both_h16(const void *x, uint8_t *codes, uint8_t *scales, uint8_t *codes_t, uint8_t *scales_t, int x_type,
                              int64_t R, int64_t K, int fmt, int rounding, uint64_t seed, uint64_t offset,
                              fp8q_stream_t stream);
int fp8q_mxsr_quantize_t_f32(const float *x, float *y, int64_t R, int64_t K, int fmt, int rounding, uint64_t seed,
                             uint64_t offset, fp8q_stream_t stream);
int fp8q_mxsr_quantize_t_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int fmt, int rounding,
                             uint64_t seed, uint64_t offset, fp8q_stream_t stream);

/* ---- hardware FP8 with seeded stochastic rounding: per tensor / channel, per tile, and the transposed operands ----------------
 * (csrc/fp8q_ocpq.h, used by csrc/fp8q_ocp.hip, csrc/fp8q_ocp_block.hip and csrc/fp8q_ocp_block_t.hip)  The operands these lanes
 * make for the backward products are gradients, and the reason the block above gives for the MX lane holds for them.  These
 * twelve entries are the twins of the OCP entries that convert elements, with `uint64_t seed, uint64_t offset` in front of
 * `stream`.  Everything up to q is the twin's contract: scale = max(maxval, eps) / fmax (in the tile lanes from the tile's own
 * amax), q = clamp(x / scale, -fmax, fmax) with x / scale the float32 IEEE quotient, a NaN q stores 0x7F, and the reported
 * scales are unchanged.  Only
 *   code = RNE(q)   becomes   code = RNE(SR(q, r))
 * with SR the rounding of the block above for E4M3FN (M = 3, B = 7) and E5M2 (M = 2, B = 15) -- the 16 bits under the kept
 * mantissa in the normal range, the one truncated float32 product in the format-subnormal range, the sign kept on a zero too,
 * fmax a grid point that nothing passes -- and r the 16-bit draw of the block above: key from seed, counter from g = i >> 3,
 * word (i >> 1) & 3, half i & 1, where i = offset + the flat index of the element in x AS IT LIES mod 2^64 (the transposed
 * entries index by the position in x, not in x^T; for [R, K] that is offset + row * K + col).
 * What follows: grid points never move; every result is one of q's two grid neighbours; P(away from zero) =
 * floor(f * 2^16) / 2^16; quantize(seed) == decode(encode(seed)); encode_both(seed) == (encode(seed), encode_t(seed)), and at
 * (128, 128) codes_t is still the transpose of codes; a slice encoded under the same scale with the offset of its first
 * element (a multiple of 8) equals the slice of the whole.
 * The quotient.  The round-to-nearest-even kernels never form fl32(x / scale): they convert the two ends of an interval around
 * x * (1 / scale) and redo a dword by division where the ends disagree.  SR reads every bit of the quotient -- a wrong last
 * bit moves f16 by one and can flip a code -- so these kernels take the IEEE division for every element.
 * Errors are the twin's, all reported before the launch; an offset that is no multiple of 8 is FP8Q_EINVAL.  Routes
 * (fp8q_chunk_route, fp8q_ocpb_route, fp8q_ocpbt_route), launch geometry and traffic are the twin's.  gfx950's own stochastic
 * conversions (v_cvt_sr_*) are not used: they take 32 random bits and are unproven against this contract, the decision the MX
 * lane made.
 * Names: fp8q_ocpsr_*, fp8q_ocpbsr_*, fp8q_ocpbtsr_*; the sets of fp8q_ocp_*, fp8q_ocpb_* and fp8q_ocpbt_* entries are
 * unchanged.  FP8Q_VERSION is unchanged: the entries are additive. */
int fp8q_ocpsr_encode_f32(const float *x, uint8_t *codes, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval,
                          int fmt, float eps, float *scale_out, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpsr_encode_h16(const void *x, uint8_t *codes, int x_type, int64_t C, int64_t inner, const float *maxval,
                          int64_t n_maxval, int fmt, float eps, float *scale_out, uint64_t seed, uint64_t offset,
                          fp8q_stream_t stream);
int fp8q_ocpsr_quantize_f32(const float *x, float *y, int64_t C, int64_t inner, const float *maxval, int64_t n_maxval, int fmt,
                            float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpsr_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t C, int64_t inner, const float *maxval,
                            int64_t n_maxval, int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpbsr_encode_f32(const float *x, uint8_t *codes, float *scales, int64_t R, int64_t K, int tile_r, int tile_k, int fmt,
                           float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpbsr_encode_h16(const void *x, uint8_t *codes, float *scales, int x_type, int64_t R, int64_t K, int tile_r,
                           int tile_k, int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpbsr_quantize_f32(const float *x, float *y, int64_t R, int64_t K, int tile_r, int tile_k, int fmt, float eps,
                             uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpbsr_quantize_h16(const void *x, void *y, int x_type, int y_type, int64_t R, int64_t K, int tile_r, int tile_k,
                             int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpbtsr_encode_f32(const float *x, uint8_t *codes_t, float *scales_t, int64_t R, int64_t K, int tile_r, int tile_k,
                            int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpbtsr_encode_h16(const void *x, uint8_t *codes_t, float *scales_t, int x_type, int64_t R, int64_t K, int tile_r,
                            int tile_k, int fmt, float eps, uint64_t seed, uint64_t offset, fp8q_stream_t stream);
int fp8q_ocpbtsr_encode_both_f32(const float *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int64_t R,
                                 int64_t K, int tile_r, int tile_k, int fmt, float eps, uint64_t seed, uint64_t offset,
                                 fp8q_stream_t stream);
int fp8q_ocpbtsr_encode_both_h16(const void *x, uint8_t *codes, float *scales, uint8_t *codes_t, float *scales_t, int x_type,
                                 int64_t R, int64_t K, int tile_r, int tile_k, int fmt, float eps, uint64_t seed,
                                 uint64_t offset, fp8q_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FP8Q_H */
