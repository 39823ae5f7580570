"""The large regime of the streaming kernels, reached by size: every tensor here is at or just above the default
nontemporal threshold (kNtBytes = 64 MiB, fp8q_common.h) and at most ~1 % above it, so the `NT = true` template instances,
the one-16-KiB-piece-per-block grid rule and the staged epilogue kernel k_affine_act<true, 4> run -- at odd row lengths,
ragged last pieces, 16-byte groups that cross planes, rows at every 4-byte phase and more images than gridDim.y.

Every comparison is bit for bit against the lane's high-precision reference over the WHOLE output (NaN masks and integer
views compared separately), and, where the op is row- / image- / element-separable, a contiguous slice of the same input
goes through the same fp8q.ops call below 64 MiB (the small regime) and must give the bits of the large result.  NaN, +-inf
and -0.0 sit in the first 16-byte group, the last group, the last partial piece and right behind a 16 KiB piece border
(min/max ops: finite extremes and -0.0 there, so that a dropped tail moves the range).  No environment variable is set;
each test first asserts that FP8Q_NT_MB is unset or 64.

Audit of the `nt` / large-grid decisions of csrc/fp8q_quant.hip: is there a test under tests/ that crosses 64 MiB on the
route with a row length that is no multiple of 4 AND a channel count that does not divide the grid?

  decision (launcher)                          crossed by                                        odd rows, ragged C   here
  launch_rows_flat  k_rows_flat<Quant, NT>     test_full_size_properties [2^20,147]: 4096 rows    147 yes, C = 2^20 no  99, 1153
                                               spot-checked; test_hip_parity.py
  launch_rows_flat  k_rows_staged<NT>          test_hip_parity.py::test_staged_fused_short_rows_  yes: [200003,147],    covered: not
                                               many_chunks, whole output and ranges vs the oracle [90001,201], [70001,  added
                                                                                                  255] (72..118 MB)
  launch_rows_staged_mm  k_rows_staged_mm<NT>  test_full_size_properties (ranges of the fused)    147 yes, C = 2^20 no  201
  launch_rows_reg  k_rows_reg<.., NT, quant>   test_baseline_size.py config-5 slabs: rows are     no                    388
                                               multiples of 4
  launch_rows_direct  k_rows_direct<.., NT>    none above 64 MiB (fused rows of 257..16384)       no                    8197
  fp8q_quantize_f32  k_quant_rows<true, 4>     test_more_than_2_31_elements: three 64 Ki windows  odd n; may skip on    odd n, all
                     (per tensor)              against the small regime, the tail vs the oracle   free HBM              elements
  fp8q_quantize_f32  k_quant_rows<true, 4>     test_more_than_2_31_elements [2, n/2]: one window  no                    [2047, 8197]
                     (per channel, long rows)
  fp8q_quantize_f32  k_quant_scalar + the      none above 64 MiB                                  no                    out= off by
                     large-grid block cap                                                                               one element
  minmax_impl  k_minmax_partial<true>          test_spin_waiting... [64,64,112,112] per tensor,   no                    [2047, 8197]
                                               test_more_than_2_31_elements (planted extremes)
  quantize_sel_launch / fp8q_quantize_select_  test_baseline_size.py (model activations at        no                    not added: the
  f32 (device-resident width / sign)           batch 64, friendly shapes)                                               geometry code is
                                                                                                                        fp8q_quantize_f32's
  plan_build (`nelem * 4 < kNtBytes`)          not a kernel decision: tensors from 64 MiB leave the batched launch and take
                                               fp8q_quantize_f32 / the codec entry points, which the rows above cover
  launch_codec_flat  k_rows_flat<En/Decode>    test_hip_codec_short_row_geometries stays below    no                    not in this
                                               64 MiB ((70001, 147) = 41 MB)                                            issue's list

What ops.rows_route (fp8q_rows_route: the launchers' own decision code) shows of the row kernels' nontemporal instances, and
which the cases here now assert before they compare (kernel, nontemporal, and the launcher's choices):
  k_rows_flat<Quant, true>       test_fp32_rows_flat: resident grid of 1024 blocks, 2 and 4 chunks per tile; also the first four
                                 shapes of test_hip_parity.py::test_flat_kernel_resident_grid_mid_size (77 MB and more)
  k_rows_staged<true>            test_hip_parity.py::test_staged_fused_short_rows_many_chunks (route asserted there)
  k_rows_flat<Fused, true>       was reached by nothing: the two-pass fused kernel needs rows of at most 256 elements whose staged
                                 window plus tables exceed 36 KiB -- 129-entry tables (seven exponent bits) or, with E5M2, rows
                                 of about 64 elements and fewer -- in a tensor of 64 MiB.  Added: test_fp32_fused_rows_flat
                                 [275037, 61].  Its cached instance: tests/test_rows_routes_gpu.py
  k_rows_staged_mm<true>, k_rows_reg<.., true, quant and K2>, k_rows_direct<Fused, lut, true>, k_minmax_partial<true>,
  k_quant_rows<true, 4> per channel and per tensor: test_fp32_fused_rows, test_fp32_per_tensor (asserted)
  k_rows_direct<Quant, .., true>, k_rows_direct<Fused, no tables, true>: reached by nothing above 64 MiB (rows shorter than
                                 2 * (pmax + 1) elements, or pointers off a 16-byte boundary, at that size)
  the slab loop of k_quant_rows (C > 65535 rows of 2048 elements and more: at least 0.5 GB): reached by nothing;
                                 test_more_than_2_31_elements has two rows.  The query reports its launches by arithmetic
                                 (tests/test_rows_routes_host.py)

Also seen while auditing: tests/test_h16_kernels.py::test_streaming_sizes already crosses the half lane's threshold with
[228263, 147] (quantize only), and tests/test_int_kernels.py::test_bulk_tensor crosses the INT lane's with [2^21, 3, 7, 7]
(int_quantize, 8 bits); the cases below add the other ops, widths and shapes of those lanes.

The uniform (INT) reference is the quantizers' own torch op chain (quantization/uniform.py) on the same device, selected
without a switch: a quantizer whose discretizer is a wrapper around round_ste_func is off the kernel path.
"""
import gc
import os

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

NT_BYTES = 64 << 20                 # default kNtBytes
PIECE_BYTES = 16 << 10              # one piece: kBlock lanes x 4 loads x 16 bytes
SPECIAL = (float("nan"), float("inf"), -0.0, float("-inf"))


def _ops():
    from fp8q import ops
    return ops


def _guard(nbytes):
    """the default threshold is in force and this tensor is in the large regime, by at most ~1 %"""
    v = os.environ.get("FP8Q_NT_MB")
    assert v is None or v.strip() == "64", f"FP8Q_NT_MB={v!r}: these tests need the default 64 MiB threshold"
    assert NT_BYTES <= nbytes <= NT_BYTES * 1.01, nbytes


def _below(t):
    """a slice twin must run the small regime"""
    assert 0 < t.numel() * t.element_size() < NT_BYTES
    return t


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _probe_offsets(n, piece):
    """first 16-byte group, first elements behind the first piece border, start of the last (partial) piece, last group --
    of a range of n elements cut into pieces of `piece` elements"""
    last_piece = (n - 1) // piece * piece
    want = list(range(4)) + list(range(piece, piece + 4)) + list(range(last_piece, last_piece + 4)) + list(range(n - 4, n))
    return sorted({i for i in want if 0 <= i < n})


def _probes(shape, itemsize=4, rows=None):
    """flat indices of the probes: of the whole tensor (the kernels that cut the flat tensor into aligned pieces) and of
    some rows / images (the kernels whose pieces are relative to a row: k_quant_rows, k_codec_rows, the epilogue)"""
    n = int(np.prod(shape))
    piece = PIECE_BYTES // itemsize
    idx = set(_probe_offsets(n, piece))
    if len(shape) > 1:
        C = shape[0]
        inner = n // C
        for r in ((1, C - 1) if rows is None else rows):
            if 0 <= r < C:
                idx.update(r * inner + o for o in _probe_offsets(inner, piece))
    return torch.tensor(sorted(idx), dtype=torch.int64)


def _plant(x, idx, special):
    """special: NaN, +inf, -0.0, -inf in turn; else finite extremes that grow towards the end (+(100 + k), -(100 + k), -0.0,
    50 + k): the tensor's and the last row's maximum and minimum then sit in the last 16-byte group"""
    k = torch.arange(idx.numel(), dtype=torch.float32)
    if special:
        vals = torch.tensor(SPECIAL)[torch.arange(idx.numel()) % 4]
    else:
        vals = torch.stack([100.0 + k, -(100.0 + k), torch.full_like(k, -0.0), 50.0 + k])[torch.arange(idx.numel()) % 4,
                                                                                           torch.arange(idx.numel())]
    x.view(-1)[idx.to(x.device)] = vals.to(device=x.device, dtype=x.dtype)
    return x


def _randn(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, device="cuda", generator=g)
    if scale != 1.0:
        x *= scale
    return x if dtype == torch.float32 else x.to(dtype)


def _check(got, ref, what):
    """bit for bit: NaN at the same places, equal integer views elsewhere (integer tensors: equal)"""
    got = got.detach().cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    ref = ref.detach().cpu() if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref))
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    got, ref = got.contiguous(), ref.contiguous()
    if got.is_floating_point():
        it = {4: torch.int32, 2: torch.int16}[got.element_size()]
        nan = ref.isnan()
        bad = (got.isnan() != nan) | ((got.view(it) != ref.view(it)) & ~nan)
    else:
        bad = got != ref
    n_bad = int(bad.sum())
    if n_bad:
        first = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {n_bad} of {bad.numel()} elements differ, the first at flat index {first}: "
                             f"got {got.reshape(-1)[first].item()!r}, expected {ref.reshape(-1)[first].item()!r}")


def _np(t):
    return t.detach().cpu().numpy()


def _out(like, dtype=torch.float32):
    """an out= tensor filled with a sentinel (NaN; 0x5a.. for codes): an element the kernel does not write cannot pass by
    holding what an earlier launch left in recycled device memory"""
    fill = float("nan") if dtype.is_floating_point else (0x5a if dtype == torch.uint8 else 0x5a5a)
    return torch.full(tuple(like.shape), fill, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------------------------
# 1. the fused epilogue: k_affine_act<true, 4> (affine_quantize_impl: N * image * 4 >= kNtBytes) and the min/max twin
# ------------------------------------------------------------------------------------------------------------------
EPI_SHAPES = [
    # 67.2 MB; image = 524656, 128 whole pieces + 92 groups; affine_grid: pieces * by = 4096 <= 4096 -> the resident rule,
    # grid (64, 32), two steps per block + block 0's ragged third; HW = 121: cpp = 35 planes per piece staged in LDS per step,
    # magic division of the piece-local offset, groups cross planes
    (32, 4336, 11, 11),
    # 67.2 MB; image = 1024 (a quarter piece: the tail branch only), grid (1, 16400); HW = 1: cpp = min(4096, C) = 1024
    # planes staged, every element of a group its own plane
    (16400, 1024),
    # 67.4 MB; image = 1870964 = 456 pieces + 797 groups; pieces * by = 4104 > 4096 -> one piece per block, grid (456, 9),
    # block 0 takes the ragged piece; HW = 16129 >= 4096: cpp = 2, the two-planes-in-registers path (direct)
    (9, 116, 127, 127),
    # 67.2 MB; one image of 4100 pieces + 753 groups, grid (4100, 1); HW = 247009 > kMagicMaxDivisor: cpp = 2, direct
    # path with compare instead of divide (a.magic = 0)
    (1, 68, 497, 497),
    # 67.2 MB; 70000 images > 65535: two launches (65535 + 4465 images), x / y / residual offset per slab; image = 240:
    # 60 groups, tail branch; HW = 4: cpp = min(1025, C) = 60
    (70000, 60, 2, 2),
]
EPI_COMBOS = [(True, False, 1), (True, True, 1), (False, True, 0), (True, False, 2), (False, False, 0)]
EPI_IDS = ["bn_relu", "bn_res_relu", "res_only", "bn_relu6", "plain"]


@pytest.mark.parametrize("use_bn,use_res,act", EPI_COMBOS, ids=EPI_IDS)
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_epilogue(shape, use_bn, use_res, act):
    ops = _ops()
    n = int(np.prod(shape))
    _guard(n * 4)
    N, C = shape[0], shape[1]
    seed = 1000 * EPI_SHAPES.index(shape) + 10 * act + 2 * use_bn + use_res
    x = _randn(shape, seed, 2.0)
    assert ops.affine_act_supported(x)
    # pieces are relative to an image: probes in the first two images, the last, and on both sides of the slab border
    idx = _probes((N, n // N), rows=(0, 1, N - 1, 65534, 65535))
    _plant(x, idx, True)
    res = _randn(shape, seed + 1) if use_res else None
    rng = np.random.RandomState(seed)
    bn = bnd = ab = None
    if use_bn:
        var = (rng.rand(C) + 0.5).astype(np.float32)
        invstd = (np.float32(1) / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
        bn = (rng.randn(C).astype(np.float32), invstd, (rng.rand(C) + 0.5).astype(np.float32), rng.randn(C).astype(np.float32))
        bnd = tuple(torch.from_numpy(b).cuda() for b in bn)
        ab = ops.bn_fold(bnd)
        _check(ab[:, 0], torch.from_numpy(bn[1] * bn[2]), "bn_fold alpha")
    mv = np.array([2.5], np.float32)
    mvd = torch.from_numpy(mv).cuda()
    xh = _np(x)
    resh = _np(res) if use_res else None
    t = oracle.c_affine_act(xh, bn, resh, act)
    ref = torch.from_numpy(oracle.c_quantize(t, mv, 3, 8, 1))                         # E4M3, per tensor

    y = ops.affine_act_quantize(x, mvd, 3, 8, 1, bn=bnd, residual=res, act=act, out=_out(x)).cpu()
    _check(y, ref, "affine_act_quantize vs oracle")
    del ref
    if use_bn:      # the folded-constants entry point: the same bits
        _check(ops.affine_act_quantize(x, mvd, 3, 8, 1, bn=bnd, bn_ab=ab, residual=res, act=act, out=_out(x)), y,
               "bn_ab entry point")
    prep = ops.quantizer_prepare(mvd, 3, 8, 1)
    _check(ops.affine_act_quantize(x, mvd, 3, 8, 1, bn=bnd, bn_ab=ab, residual=res, act=act, prep=prep, out=_out(x)), y,
           "prep entry point")
    # the quantizer switched off (passthrough: the same kernel and geometry)
    _check(ops.affine_act(x, ab, res, act, out=_out(x)), torch.from_numpy(t), "affine_act vs oracle")
    del t

    # cross-regime: the last eighth of the images (one image: of the channels) through the small regime
    if N > 1:
        k = max(N // 8, 1)
        xs, rs, bns, ys = x[N - k:], (res[N - k:] if use_res else None), bnd, y[N - k:]
    else:
        k = max(C // 8, 1)
        xs, rs, ys = x[:, C - k:], (res[:, C - k:] if use_res else None), y[:, C - k:]
        bns = tuple(b[C - k:] for b in bnd) if use_bn else None
    assert xs.is_contiguous()
    _check(ops.affine_act_quantize(_below(xs), mvd, 3, 8, 1, bn=bns, residual=rs, act=act, out=_out(xs)), ys,
           "slice through the small regime")
    del y, ys, xs, rs

    # the range of the same pre-quantization tensor: finite extremes instead of the NaN / inf probes
    _plant(x, idx, False)
    t2 = oracle.c_affine_act(_np(x), bn, resh, act)
    rmn, rmx = oracle.c_minmax(t2, False)
    mn, mx, mvo = ops.affine_act_minmax(x, bn=bnd, residual=res, act=act)
    _check(mn, rmn, "affine_act_minmax min")
    _check(mx, rmx, "affine_act_minmax max")
    _check(mvo, oracle.c_absmax(rmn, rmx), "affine_act_minmax maxval")
    ops.check_workspaces()


# ------------------------------------------------------------------------------------------------------------------
# 2. FP8 storage codes of long rows: k_codec_rows<ENCODE, true> (fp8q_codec.hip codec_launch: C * inner * 4 >= kNtBytes)
# ------------------------------------------------------------------------------------------------------------------
CODEC_FORMATS = {"E5M2": (2, (57344.0, 0.7361, 3.0)), "E4M3": (3, (240.0, 0.7361, 2.5))}      # M, ranges whose tables are
#                                                             exactly geometric (tests/test_codes.py: exact round trips)
CODEC_SHAPES = [
    # 67.1 MB, per tensor: one row, grid (1366, 1), 3 steps per block; encode: 1048578 16-element words + 5 tail elements,
    # decode: 4194313 groups + 1 tail element
    ((1 << 24) + 37,),
    # 67.1 MB, per channel: inner >= 2048 -> the row kernel, grid (683, 3); rows start at byte phases 0, 12 and 8: rows 1
    # and 2 take the element-wise branch on the fp32 side
    (3, 5592407),
]


@pytest.mark.parametrize("fmt", list(CODEC_FORMATS))
@pytest.mark.parametrize("shape", CODEC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp8_storage_codes_long_rows(shape, fmt):
    ops = _ops()
    n = int(np.prod(shape))
    _guard(n * 4)
    M, ranges = CODEC_FORMATS[fmt]
    pc = len(shape) > 1
    mv = np.array(ranges if pc else ranges[:1], np.float32)
    x = _randn(shape, 7 + M)
    x *= torch.from_numpy(mv / np.float32(2.2)).cuda().view(-1, *([1] * (len(shape) - 1)))
    _plant(x, _probes(shape, rows=(0, 1, 2)), True)
    xh = _np(x)
    mvd = torch.from_numpy(mv).cuda()
    codes = ops.encode(x, mvd, M, 8, 1, out=_out(x, torch.uint8))
    assert codes.dtype == torch.uint8 and codes.shape == x.shape
    ch = codes.cpu()
    _check(ch, oracle.c_encode(xh, mv, M, 8, 1), "encode vs oracle")
    # decode(encode(x)) == quantize(x); a NaN has no code and is stored as code 0 (include/fp8q.h), which decodes to +0
    want = oracle.c_quantize(xh, mv, M, 8, 1)
    assert np.isnan(want[np.isnan(xh)]).all()
    want[np.isnan(xh)] = 0.0
    _check(ops.decode(codes, mvd, M, 8, 1, out=_out(x)), want, "decode(encode(x)) vs oracle quantize")
    # cross-regime: the last 2 Mi + 37 elements (16-byte aligned start) / the last row (8-byte phase) below 64 MiB
    if pc:
        xs, cs, ms = x[2:], ch[2:], mvd[2:]
    else:
        k = (1 << 21) + 37
        xs, cs, ms = x[n - k:], ch[n - k:], mvd
    cs_small = ops.encode(_below(xs), ms, M, 8, 1, out=_out(xs, torch.uint8))
    _check(cs_small, cs, "codes of a slice through the small regime")
    _check(ops.decode(cs_small, ms, M, 8, 1, out=_out(xs)), want[2:] if pc else want[n - k:], "decode of a slice through the small regime")


# ------------------------------------------------------------------------------------------------------------------
# 3. the half lane: fp8q_h16.hip quant_launch (`a.n * 2 >= kNtBytes`, :396) and minmax_launch (`C * inner * 2`, :461)
# ------------------------------------------------------------------------------------------------------------------
HALF = {"fp16": torch.float16, "bf16": torch.bfloat16}
HALF_SHAPES = [
    # 67.1 MB of half, per tensor: ng = 4194307 groups of 8 -> U = 4, 4097 chunks of 8192 elements, k_h16_quant<.., 4, true>;
    # min/max: one row, k_h16_minmax_part<T, true> split over 2048 blocks + the reducer
    ((1 << 25) + 24,),
    # 67.1 MB, per channel, rows of 147: U = 4 (57 table rows per chunk fit the LDS budget), magic division;
    # min/max: inner <= 2048 -> k_h16_minmax_rows (no nontemporal variant: the launcher decides by row length first)
    (228262, 147),
    # 67.1 MB, per channel, rows of 3728271 (odd: rows start at every 2-byte phase of a 16-byte group): two table rows per
    # chunk, compare instead of divide; min/max: k_h16_minmax_part<T, true>, 114 splits per row
    (9, 3728271),
]


def _half_input(shape, dtype, special, seed):
    x = _randn(shape, seed, dtype=dtype)
    return _plant(x, _probes(shape, itemsize=2), special)


def _row_ranges(C, seed):
    return (np.random.RandomState(seed).rand(C) * 2.5 + 0.5).astype(np.float32)


def _row_slice(shape, frac=8):
    """(slice of dim 0 / of the flat tensor) for the cross-regime twin: the last rows, or the last eighth of one row"""
    if len(shape) > 1:
        return slice(shape[0] - max(shape[0] // frac, 1), shape[0])
    n = shape[0]
    k = n // frac // 4096 * 4096 + n % 4096                 # the slice starts on a piece border: same alignment as the whole
    return slice(n - k, n)


@pytest.mark.parametrize("dtype", list(HALF))
@pytest.mark.parametrize("shape", HALF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_half_quantize(shape, dtype):
    ops = _ops()
    dt = HALF[dtype]
    n = int(np.prod(shape))
    _guard(n * 2)
    pc = len(shape) > 1
    M = 2 if pc else 3                                        # E5M2 for rows, E4M3 per tensor
    x = _half_input(shape, dt, True, 31)
    mv = _row_ranges(shape[0], 5) if pc else np.array([2.5], np.float32)
    mvd = torch.from_numpy(mv).cuda()
    want = torch.from_numpy(oracle.c_quantize(_np(x.float()), mv, M, 8, 1))          # the fp32 contract on the widened input
    sl = _row_slice(shape)
    y = ops.quantize(x, mvd, float(M), 8, 1, out=_out(x))
    assert y.dtype == torch.float32
    _check(y, want, "float32 result vs oracle")
    del y
    yh = ops.quantize(x, mvd, float(M), 8, 1, out=_out(x, dt))
    assert yh.dtype == dt
    _check(yh, want.to(dt), "half result vs oracle rounded once")
    del yh
    ms = mvd[sl] if pc else mvd
    _check(ops.quantize(_below(x[sl]), ms, float(M), 8, 1, out=_out(x[sl])), want[sl], "slice through the small regime")
    _check(ops.quantize(x[sl], ms, float(M), 8, 1, out=_out(x[sl], dt)), want[sl].to(dt), "slice through the small regime, half out")


@pytest.mark.parametrize("dtype", list(HALF))
@pytest.mark.parametrize("shape", HALF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_half_minmax(shape, dtype):
    ops = _ops()
    dt = HALF[dtype]
    _guard(int(np.prod(shape)) * 2)
    pc = len(shape) > 1
    x = _half_input(shape, dt, False, 32)
    xf = x.float()
    rmn, rmx = oracle.c_minmax(_np(xf), pc)
    got = ops.minmax(x, pc, want_maxval=True)
    for g, r, name in zip(got, (rmn, rmx, oracle.c_absmax(rmn, rmx)), ("min", "max", "maxval")):
        assert g.dtype == torch.float32
        _check(g, r, f"minmax {name} vs oracle")
    for g, r, name in zip(got, ops.minmax(xf, pc, want_maxval=True), ("min", "max", "maxval")):     # test_h16_kernels.py's reference
        _check(g, r, f"minmax {name} vs the float32 entry point")
    del xf
    # a second batch folded into the estimate (FOLD_ALL): the halved tensor cannot widen the range
    mn2, mx2 = ops.minmax(x * 0.5, pc, got[0].clone(), got[1].clone(), mode=ops.FOLD_ALL)
    _check(mn2, got[0], "FOLD_ALL min")
    _check(mx2, got[1], "FOLD_ALL max")
    if pc:      # rows are separable
        sl = _row_slice(shape)
        for g, r, name in zip(got, ops.minmax(_below(x[sl]), True, want_maxval=True), ("min", "max", "maxval")):
            _check(g[sl], r, f"minmax {name} of a slice through the small regime")
    ops.check_workspaces()


# minmax_quantize takes rows up to fused_max_inner() = 16384: the short odd rows, and the longest odd row it accepts
# ([2049, 16383], 67.1 MB: ranges by k_h16_minmax_part<T, true> with one block per row, then k_h16_quant<.., 4, true>)
@pytest.mark.parametrize("dtype", list(HALF))
@pytest.mark.parametrize("shape", [(228262, 147), (2049, 16383)], ids=lambda s: "x".join(map(str, s)))
def test_half_minmax_quantize(shape, dtype):
    ops = _ops()
    dt = HALF[dtype]
    _guard(int(np.prod(shape)) * 2)
    assert shape[1] <= ops.fused_max_inner()
    x = _half_input(shape, dt, False, 33)
    xh = _np(x.float())
    rmn, rmx = oracle.c_minmax(xh, True)
    rmv = oracle.c_absmax(rmn, rmx)
    want = torch.from_numpy(oracle.c_quantize(xh, rmv, 2, 8, 1))
    del xh
    y, mn, mx, mv = ops.minmax_quantize(x, 2.0, 8, 1, out=_out(x))
    assert y.dtype == torch.float32
    for g, r, name in ((mn, rmn, "min"), (mx, rmx, "max"), (mv, rmv, "maxval")):
        _check(g, r, f"row {name} vs oracle")
    _check(y, want, "float32 result vs oracle")
    del y
    yh, _, _, mvh = ops.minmax_quantize(x, 2.0, 8, 1, out=_out(x, dt))
    _check(mvh, rmv, "maxval (half out) vs oracle")
    _check(yh, want.to(dt), "half result vs oracle rounded once")
    del yh
    sl = _row_slice(shape)
    ys, _, _, mvs = ops.minmax_quantize(_below(x[sl]), 2.0, 8, 1, out=_out(x[sl]))
    _check(mvs, rmv[sl], "maxval of a slice through the small regime")
    _check(ys, want[sl], "slice through the small regime")


# ------------------------------------------------------------------------------------------------------------------
# 4. the uniform (INT) quantizers: fp8q_int.hip int_quant_launch and fp8q_intcodec.hip codec_launch, both through
#    FP8Q_INT_LAUNCH (fp8q_intq.h):
#    `a.n * 4 >= kNtBytes` with x and y 16-byte aligned -> the <.., VEC = true, NT = true> instances; one aligned
#    4096-element chunk per block (4097 blocks here, the last one ragged)
# ------------------------------------------------------------------------------------------------------------------
INT_SHAPES = [
    # 67.1 MB, per tensor: the last chunk holds 5 elements: one group + one tail scalar
    ((1 << 24) + 5,),
    # 67.1 MB, per channel, rows of 147: up to 29 rows' constants per chunk in LDS, channel by magic division
    (114131, 147),
    # 67.1 MB, per channel, rows of 3355447 >= a chunk: two rows per chunk at most, compare instead of divide
    (5, 3355447),
]


def _round_chain(t):
    from quantization.fp8 import round_ste_func
    return round_ste_func(t)


def _int_quantizers(shape, sym, n_bits, nonneg):
    """(qc, qe): qc a quantizer whose ranges the CPU chain set (the reference's arithmetic: tests/test_int_kernels.py's
    docstring); qe the same ranges on the GPU in a quantizer that runs the torch op chain there"""
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    cls = SymmetricUniformQuantizer if sym else AsymmetricUniformQuantizer
    pc = len(shape) > 1
    C = shape[0] if pc else 1
    g = torch.Generator().manual_seed(11 * n_bits + sym)
    xmin = (-torch.rand(C, generator=g) * 4) if pc else -torch.rand((), generator=g) * 4
    xmax = (torch.rand(C, generator=g) * 4) if pc else torch.rand((), generator=g) * 4
    if pc and C > 4:
        xmin[1] = xmax[1] = 0.0                     # degenerate channel
        xmin[2] = 0.25                              # positive minimum
    if nonneg:
        xmin = xmin.abs()                           # symmetric: unsigned
    qc = cls(n_bits=n_bits, per_channel=pc)
    qc.set_quant_range(xmin, xmax)
    return qc, _eager_on_gpu(qc), xmin, xmax


def _eager_on_gpu(q, delta=None, zero_float=None, signed=None):
    """a quantizer with q's (or the given) range buffers on the GPU whose forward / to_integer_forward is the torch chain"""
    qe = type(q)(n_bits=q.n_bits, per_channel=q.per_channel, discretizer=_round_chain)
    qe._delta = (q._delta if delta is None else delta).detach().clone().cuda()
    if q.symmetric:
        qe._signed = (q._signed if signed is None else signed).detach().clone().cuda().reshape(())
    else:
        qe._zero_float = (q._zero_float if zero_float is None else zero_float).detach().clone().cuda()
    assert not qe._fixed_kernel_ok(torch.empty(4, device="cuda"))
    return qe


def _int_args(qe, n_bits, sym):
    return (qe._delta, None if sym else qe._zero_float, qe._signed if sym else None, n_bits, sym, qe.eps)


def _sliced_args(args, sl, pc):
    d, z, s = args[:3]
    return ((d[sl] if pc else d), (z[sl] if (pc and z is not None) else z), s) + tuple(args[3:])


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("n_bits", [8, 4])
@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_int_quantize(shape, n_bits, sym):
    ops = _ops()
    n = int(np.prod(shape))
    _guard(n * 4)
    pc = len(shape) > 1
    qc, qe, xmin, xmax = _int_quantizers(shape, sym, n_bits, nonneg=(n_bits == 4))
    args = _int_args(qe, n_bits, sym)
    x = _randn(shape, 41 + n_bits, 3.0)
    idx = _probes(shape)
    _plant(x, idx, True)
    sl = _row_slice(shape)
    with torch.no_grad():
        ref = qe(x).cpu()                                                        # the torch chain, same device, same buffers
    # fixed ranges
    y = ops.int_quantize(x, *args, out=_out(x)).cpu()
    _check(y, ref, "int_quantize vs the torch chain")
    del ref
    _check(ops.int_quantize(_below(x[sl]), *_sliced_args(args, sl, pc), out=_out(x[sl])), y[sl], "slice through the small regime")
    # range + quantize in one launch: the CPU chain's range buffers, the fixed-range result
    y2, d2, z2, s2 = ops.int_range_quantize(x, xmin.cuda(), xmax.cuda(), n_bits, sym, out=_out(x))
    _check(d2, qc._delta, "int_range_quantize delta vs the CPU chain")
    if sym:
        assert bool(s2) == bool(qc._signed)
    else:
        _check(z2, qc._zero_float, "int_range_quantize zero_float vs the CPU chain")
    _check(y2, y, "int_range_quantize vs int_quantize")
    del y, y2
    if not pc:
        return
    # row min / max + range + quantize (weights): finite extremes instead of NaN / inf
    _plant(x, idx, False)
    y3, mn, mx, d3, z3, s3 = ops.int_minmax_quantize(x, n_bits, sym, out=_out(x))
    rmn, rmx = x.view(shape[0], -1).aminmax(dim=1)
    _check(mn, rmn, "int_minmax_quantize row min")
    _check(mx, rmx, "int_minmax_quantize row max")
    q3 = type(qc)(n_bits=n_bits, per_channel=True)
    q3.set_quant_range(rmn.cpu(), rmx.cpu())
    _check(d3, q3._delta, "int_minmax_quantize delta vs the CPU chain")
    if sym:
        assert bool(s3) == bool(q3._signed)
    else:
        _check(z3, q3._zero_float, "int_minmax_quantize zero_float vs the CPU chain")
    y3 = y3.cpu()
    with torch.no_grad():
        _check(y3, _eager_on_gpu(q3, d3, z3, s3)(x), "int_minmax_quantize vs the torch chain")
    ys = ops.int_minmax_quantize(_below(x[sl]), n_bits, sym, out=_out(x[sl]))
    _check(ys[3], d3[sl], "delta of a slice through the small regime")
    if sym and bool(ys[5]) != bool(s3):
        return                                      # the sign is a property of ALL rows: such a slice is another quantizer
    _check(ys[0], y3[sl], "int_minmax_quantize slice through the small regime")
    ops.check_workspaces()


def _codes_of(t, n_bits):
    """a float tensor of integers as raw storage codes (tests/test_int_codes_kernels.py)"""
    if n_bits <= 8:
        return (t.to(torch.int32) & 255).to(torch.uint8)
    return (t.to(torch.int32) & 65535).to(torch.int32).to(torch.int16)


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("n_bits", [8, 4, 16])          # 16: two-byte codes, the other store path (8 elements per 16-byte word)
@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_int_codes(shape, n_bits, sym):
    ops = _ops()
    n = int(np.prod(shape))
    _guard(n * 4)
    pc = len(shape) > 1
    qc, qe, _, _ = _int_quantizers(shape, sym, n_bits, nonneg=(n_bits == 4))
    args = _int_args(qe, n_bits, sym)
    x = _randn(shape, 43 + n_bits, 3.0)
    _plant(x, _probes(shape), True)
    sl = _row_slice(shape)
    sargs = _sliced_args(args, sl, pc)
    with torch.no_grad():
        t_ref = qe.to_integer_forward(x)
        zp = qe._params_like(x)[1]
        zp = torch.zeros((), device="cuda") if sym else zp
        want_codes = _codes_of(torch.where(t_ref.isnan(), zp.nan_to_num(0.0).expand_as(t_ref), t_ref), n_bits).cpu()
        t_ref = t_ref.cpu()
        y_ref = qe(x).cpu()
    # to_integer == the torch chain
    t = ops.int_to_integer(x, *args, out=_out(x)).cpu()
    _check(t, t_ref, "int_to_integer vs the torch chain")
    _check(ops.int_to_integer(_below(x[sl]), *sargs, out=_out(x[sl])), t[sl], "int_to_integer slice through the small regime")
    del t, t_ref
    # encode == those integers in the storage type; NaN stores the code of zp
    cdt = torch.int16 if n_bits > 8 else torch.uint8
    codes = ops.int_encode(x, *args, out=_out(x, cdt))
    assert codes.dtype == cdt and codes.shape == x.shape
    _check(codes, want_codes, "int_encode vs the torch chain's integers")
    cs = ops.int_encode(x[sl], *sargs, out=_out(x[sl], cdt))
    _check(cs, want_codes[sl], "int_encode slice through the small regime")
    del want_codes
    # decode(encode(x)) == the quantizer's forward wherever x is not NaN (a NaN decodes to the value of zp's code: 0)
    y_ref = torch.where(x.isnan().cpu(), torch.zeros(()), y_ref)
    yd = ops.int_decode(codes, *args, out=_out(x)).cpu()
    _check(torch.where(x.isnan().cpu(), torch.zeros(()), yd), y_ref, "int_decode(int_encode(x)) vs the torch chain")
    _check(ops.int_decode(cs, *sargs, out=_out(x[sl])), yd[sl], "int_decode slice through the small regime")


# ------------------------------------------------------------------------------------------------------------------
# 5. the float32 FP8 routes of fp8q_quant.hip the audit (module docstring) found uncovered
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset_out", [False, True], ids=["k_quant_rows", "k_quant_scalar"])
def test_fp32_per_tensor(offset_out):
    """fp8q_quantize_f32, C == 1, nt.  n = 4097 pieces + 1029 elements (67.1 MB): pieces * C = 4097 > 4096 -> one 16 KiB
    piece per block (cap 65536, grid 4097); k_quant_rows<true, 4>: the partial last piece (257 groups + 1 scalar) has no block
    of its own.  offset_out: out= starts one element behind a 16-byte boundary, x on one -> not co-aligned ->
    k_quant_scalar with the large regime's block cap (bs = min(cdiv(n, 256), 4 * 65536) = 65557 blocks)."""
    ops = _ops()
    n = 4097 * 4096 + 1029
    _guard(n * 4)
    x = _plant(_randn((n,), 51, 2.0), _probes((n,)), True)
    mv = np.array([2.5], np.float32)
    mvd = torch.from_numpy(mv).cuda()
    want = torch.from_numpy(oracle.c_quantize(_np(x), mv, 3, 8, 1))                    # E4M3
    out = _out(x)
    if offset_out:
        out = torch.full((n + 1,), float("nan"), device="cuda")[1:]
        assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    r = _route(ops, "quantize", x, 3, out, per_channel=False)
    assert (r["kernel"], r["nontemporal"]) == (("k_quant_scalar", False) if offset_out else ("k_quant_rows", True)), r
    assert r["grid_x"] == (65557 if offset_out else 4097), r
    y = ops.quantize(x, mvd, 3, 8, 1, out=out)
    _check(y, want, "quantize vs oracle")
    del y, out
    sl = _row_slice((n,))
    outs = torch.full((sl.stop - sl.start + 1,), float("nan"), device="cuda")[1:] if offset_out else _out(x[sl])
    _check(ops.quantize(_below(x[sl]), mvd, 3, 8, 1, out=outs), want[sl], "slice through the small regime")


def _route(ops, op, x, M, out=None, per_channel=True):
    """ops.rows_route for the call about to be made on x: kernel and launcher choices from the real pointers' phases"""
    C = x.shape[0] if per_channel and x.dim() > 1 else 1
    return ops.rows_route(op, C, x.numel() // C, per_channel, M, 8, 1, x_mod16=x.data_ptr() % 16,
                          y_mod16=(out.data_ptr() % 16) if out is not None else 0)


def _rows_case(inner, seed, special):
    C = -(-(1 << 24) // inner)                       # the fewest rows that reach 2^24 elements
    _guard(C * inner * 4)
    x = _plant(_randn((C, inner), seed), _probes((C, inner)), special)
    return C, x


@pytest.mark.parametrize("inner", [99, 1153])
def test_fp32_rows_flat(inner):
    """fp8q_quantize_f32 per channel, inner <= 2047 -> launch_rows_direct -> launch_rows_flat(kModeQuant): n * 4 >= kNtBytes ->
    k_rows_flat<kModeQuant, true>; 4097 chunks of 4096 elements (the last ragged, then C * inner % 4 = 1 or 3 tail scalars),
    <= 16384 chunks -> a resident grid of 1024 blocks striding over tiles.
    [169467, 99] (67.1 MB): 43 table rows per chunk, tiles of 2 chunks; [14551, 1153] (67.1 MB): 5 table rows, tiles of 4."""
    ops = _ops()
    C, x = _rows_case(inner, 52, True)
    mv = _row_ranges(C, inner)
    mvd = torch.from_numpy(mv).cuda()
    want = torch.from_numpy(oracle.c_quantize(_np(x), mv, 2, 8, 1))                    # E5M2
    out = _out(x)
    r = _route(ops, "quantize", x, 2, out)
    assert (r["kernel"], r["nontemporal"], r["grid_x"], r["nch"]) == ("k_rows_flat", True, 1024, 2 if inner == 99 else 4), r
    _check(ops.quantize(x, mvd, 2, 8, 1, out=out), want, "quantize vs oracle")
    del out
    sl = _row_slice((C, inner))
    _check(ops.quantize(_below(x[sl]), mvd[sl], 2, 8, 1, out=_out(x[sl])), want[sl], "slice through the small regime")


def test_fp32_fused_rows_flat():
    """fp8q_minmax_quantize_f32 just above 64 MiB on rows too short for k_rows_staged: [275037, 61] (67.1 MB), E5M2.  68 table
    rows per chunk x (33 entries + constants) next to the 18 KiB window exceed the 36 KiB a staged block may take ->
    launch_rows_flat's two-pass k_rows_flat<kModeFused, true>: 4097 chunks, one per tile and block (the fused grid is not
    the resident one), 4 lanes per row in the range pass, the last chunk ragged with one tail scalar; rows of 61 elements start
    at every 4-byte phase, so nearly every row has a head patch."""
    ops = _ops()
    inner = 61
    C, x = _rows_case(inner, 54, False)
    xh = _np(x)
    rmn, rmx = oracle.c_minmax(xh, True)
    rmv = oracle.c_absmax(rmn, rmx)
    want = torch.from_numpy(oracle.c_quantize(xh, rmv, 2, 8, 1))                       # E5M2
    del xh
    out = _out(x)
    r = _route(ops, "minmax_quantize", x, 2, out)
    assert (r["kernel"], r["nontemporal"], r["nch"], r["group"], r["grid_x"]) == ("k_rows_flat", True, 1, 4, 4097), r
    y, mn, mx, mv = ops.minmax_quantize(x, 2, 8, 1, out=out)
    for g, ref, name in ((mn, rmn, "min"), (mx, rmx, "max"), (mv, rmv, "maxval")):
        _check(g, ref, f"minmax_quantize row {name} vs oracle")
    _check(y, want, "minmax_quantize vs oracle")
    del y, out
    sl = _row_slice((C, inner))
    ys, _, _, mvs = ops.minmax_quantize(_below(x[sl]), 2, 8, 1, out=_out(x[sl]))
    _check(ys, want[sl], "slice through the small regime")
    _check(mvs, rmv[sl], "maxval of a slice through the small regime")


@pytest.mark.parametrize("inner", [388, 201, 8197])
def test_fp32_fused_rows(inner):
    """fp8q_minmax_quantize_f32 and fp8q_minmax_f32 (per channel) just above 64 MiB:
    [43241, 388] (67.1 MB): rows of 128..8192, a multiple of 4 -> launch_rows_reg: 16 lanes x 7 slots (87 % filled),
        k_rows_reg<16, 7, true, true>, 2703 blocks of 16 rows, the last with 9; min/max alone: k_rows_reg<16, 7, true, false>.
    [83469, 201] (67.1 MB): min/max alone only -- rows_reg's fill is 79.6 % < 80 % -> launch_rows_staged_mm ->
        k_rows_staged_mm<true>, 4097 chunks, one per block, the last ragged with one tail scalar.  (The fused call on such rows
        is k_rows_staged<true>, which test_hip_parity.py::test_staged_fused_short_rows_many_chunks covers above 64 MiB.)
    [2047, 8197] (67.1 MB): > 8192 -> not rows_reg, > 256 -> not flat -> k_rows_direct<kModeFused, true, true>; min/max
        alone: > 2047 -> k_minmax_partial<true>, one block per row; quantize with those ranges: > 2047 -> k_quant_rows<true, 4>
        per channel, grid (1, 2047) by the resident rule (pieces * C = 4094 <= 4096: 2048 blocks in all, one per row), rows at every 4-byte phase."""
    ops = _ops()
    C, x = _rows_case(inner, 53, False)
    assert inner <= ops.fused_max_inner()
    xh = _np(x)
    rmn, rmx = oracle.c_minmax(xh, True)
    rmv = oracle.c_absmax(rmn, rmx)
    want = torch.from_numpy(oracle.c_quantize(xh, rmv, 2, 8, 1))                       # E5M2
    del xh
    fused = inner != 201
    r = _route(ops, "minmax", x, 2)
    assert r["nontemporal"] and r["kernel"] == {388: "k_rows_reg", 201: "k_rows_staged_mm", 8197: "k_minmax_partial"}[inner], r
    if inner == 388:
        assert (r["lanes"], r["slots"]) == (16, 7), r
    if fused:
        out = _out(x)
        r = _route(ops, "minmax_quantize", x, 2, out)
        assert (r["kernel"], r["nontemporal"]) == ("k_rows_reg" if inner == 388 else "k_rows_direct", True), r
        assert (r["lanes"], r["slots"], r["lut"]) == ((16, 7, False) if inner == 388 else (0, 0, True)), r
        y, mn, mx, mv = ops.minmax_quantize(x, 2, 8, 1, out=out)
        del out
        for g, r, name in ((mn, rmn, "min"), (mx, rmx, "max"), (mv, rmv, "maxval")):
            _check(g, r, f"minmax_quantize row {name} vs oracle")
        _check(y, want, "minmax_quantize vs oracle")
        del y
    for g, r, name in zip(ops.minmax(x, True, want_maxval=True), (rmn, rmx, rmv), ("min", "max", "maxval")):
        _check(g, r, f"minmax row {name} vs oracle")
    if inner > 2047:
        r = _route(ops, "quantize", x, 2, x)
        assert (r["kernel"], r["nontemporal"], r["grid_x"], r["grid_y"]) == ("k_quant_rows", True, 1, 2047), r
        _check(ops.quantize(x, mv, 2, 8, 1, out=_out(x)), want, "quantize (long rows, per channel) vs oracle")
    sl = _row_slice((C, inner))
    if fused:
        ys, _, _, mvs = ops.minmax_quantize(_below(x[sl]), 2, 8, 1, out=_out(x[sl]))
        _check(ys, want[sl], "slice through the small regime")
    else:
        mvs = ops.minmax(_below(x[sl]), True, want_maxval=True)[2]
    _check(mvs, rmv[sl], "maxval of a slice through the small regime")
    ops.check_workspaces()
