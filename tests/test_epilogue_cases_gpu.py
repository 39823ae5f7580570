"""The fused FP8 epilogue (csrc/fp8q_epilogue.hip: k_affine_act<NT, U>, k_affine_act_small, k_quantizer_prepare,
k_affine_minmax) against the oracle at every format, at the edges of every range, on every plane route and through every fold.

Inputs come from tests/epilogue_cases.py (tests/test_epilogue_cases_host.py proves on the CPU that their hard values reach
the quantizer); the pre-quantizer tensor is always oracle.c_affine_act's, the quantized one oracle.c_quantize's, ranges
oracle.c_minmax / c_fold / c_absmax.  The contract is bit equality -- identical NaN masks, identical int32 bits elsewhere,
the sign of zero included -- so no tolerance appears here.  Every test asserts the kernel its shape reaches
(ops.affine_act_route) before it runs; no test sets an FP8Q_* variable, so k_affine_act<false, 4> (reachable only through
FP8Q_EPI_SMALL_M) is out of scope and k_affine_act<true, 4> keeps its coverage in tests/test_large_regime.py."""
import numpy as np
import pytest
import torch

import oracle
import epilogue_cases as ec
from test_ranges_exchange import _expect_packed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import fp8q
    fp8q.lib()  # raises if libfp8q_hip.so is missing: no fallback
    return fp8q.ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def fmt_id(fmt):
    return "m%g_n%d_s%d" % fmt


def assert_route(ops, shape, has_bn):
    N, C, HW = ec.nchw(shape)
    r = ops.affine_act_route(N, C, HW, has_bn)
    assert (r["kernel"], r["direct"], r["launches"]) == ec.SHAPES[shape][bool(has_bn)], (shape, has_bn, r)


def check_quantize(ops, case, act, fmt, maxval, what):
    """affine_act_quantize from the four BN vectors, from bn_fold and with the prepared quantizer == c_quantize(t), and
    affine_act == t, bit for bit"""
    mbits, n_bits, sign_bits = fmt
    t = ec.expected_t(case, act)
    mv = np.array([maxval], np.float32)
    ref = oracle.c_quantize(t, mv, mbits, n_bits, sign_bits)
    x, mvd = dev(case["x"]), dev(mv)
    res = dev(case["res"]) if case["res"] is not None else None
    bn = tuple(dev(b) for b in case["bn"]) if case["bn"] is not None else None
    ab = ops.bn_fold(bn) if bn is not None else None
    y = ops.affine_act_quantize(x, mvd, mbits, n_bits, sign_bits, bn=bn, residual=res, act=act).cpu().numpy()
    assert ec.same_bits(y, ref), (what, "bn vectors")
    if bn is not None:
        y = ops.affine_act_quantize(x, mvd, mbits, n_bits, sign_bits, bn=bn, bn_ab=ab, residual=res, act=act).cpu().numpy()
        assert ec.same_bits(y, ref), (what, "bn_fold")
    prep = ops.quantizer_prepare(mvd, mbits, n_bits, sign_bits)
    y = ops.affine_act_quantize(x, mvd, mbits, n_bits, sign_bits, bn_ab=ab, residual=res, act=act, prep=prep).cpu().numpy()
    assert ec.same_bits(y, ref), (what, "prep")
    tt = ops.affine_act(x, ab, res, act).cpu().numpy()
    assert ec.same_bits(tt, t), (what, "affine_act")


def run_case(ops, shape, fmt, maxval, flags):
    use_bn, use_res, act = flags
    assert_route(ops, shape, use_bn)
    scale = maxval if ec.is_plain(maxval) else 1.0
    # (a tensor smaller than the edge list takes it window by window, each window at the four phases of a group)
    for r, start in enumerate(ec.starts(shape, len(ec.edge_values(fmt[0], scale, fmt[2], fmt[1])))):
        case = ec.case_input(shape, fmt, maxval, use_bn, use_res, seed=17 * r + act, start=start)
        check_quantize(ops, case, act, fmt, maxval, (shape, fmt, maxval, flags, start))


def test_routes(ops):
    """every shape of the table reaches the kernel, the constants' home and the number of launches the table says"""
    for shape in ec.SHAPES:
        for has_bn in (True, False):
            assert_route(ops, shape, has_bn)


@pytest.mark.parametrize("shape", [(2, 8, 5, 5), (3, 12, 1, 1), (5, 2, 2, 1)])
@pytest.mark.parametrize("fmt", ec.FORMATS, ids=fmt_id)
def test_formats_and_ranges(ops, fmt, shape):
    """every format x every range of it, one shape per route class, behind BN + ReLU and behind BN + residual without an
    activation (so that negatives reach the unsigned formats)"""
    for maxval in ec.ranges(fmt):
        for flags in ((True, False, 1), (True, True, 0)):
            run_case(ops, shape, fmt, maxval, flags)


# every shape x the six flag sets; the many-images shape with two of them, one with and one without the batch norm
SHAPE_FLAGS = [(s, f) for s in ec.SHAPES for f in ec.FLAGS if s[0] <= 65535 or f in ((True, True, 1), (False, False, 0))]


@pytest.mark.parametrize("shape,flags", SHAPE_FLAGS, ids=lambda v: "x".join(str(int(i)) for i in v))
def test_shapes_and_flags(ops, shape, flags):
    for fmt in ((2, 8, 1), (3, 8, 0)):
        for maxval in (ec.default_maxval(fmt), 0.7361):
            run_case(ops, shape, fmt, maxval, flags)


def check_range(got, ref_mn, ref_mx, what):
    mn, mx, mv = (t.cpu().numpy() for t in got)
    assert ec.same_bits(mn, ref_mn) and ec.same_bits(mx, ref_mx), (what, mn, mx, ref_mn, ref_mx)
    assert ec.same_bits(mv, oracle.c_absmax(ref_mn, ref_mx)), (what, "maxval_out")
    return mn, mx


@pytest.mark.parametrize("flags", [(True, True, 1), (True, False, 0), (False, True, 0)], ids=lambda f: "bn%d_res%d_act%d" % f)
@pytest.mark.parametrize("shape", [(2, 8, 5, 5), (6, 4, 3, 1), (5, 2, 2, 1)], ids=lambda s: "x".join(map(str, s)))
def test_range_twin_folds(ops, shape, flags):
    """affine_act_minmax: mode 0 is c_minmax of t; modes 1 and 2 fold three successive batches exactly as c_fold folds the
    oracle's per-batch ranges (`first` as the Python layer passes it: on the call without a running estimate); maxval_out is
    c_absmax; the packed record is what the exchange expects; NaN and +-inf in the input reach the range as c_minmax says"""
    use_bn, use_res, act = flags
    # (the quantizing kernels' route, asserted as everywhere in this file: the shape classes are theirs.  k_affine_minmax
    # itself does not go through affine_dispatch -- its grid is affine_grid's read-only arm -- so this says nothing about it)
    assert_route(ops, shape, use_bn)
    fmt = (3, 8, 1)
    numel = int(np.prod(shape))
    batches = []
    for i, mvb in enumerate((2.5, 0.7361, 31.0)):
        case = ec.case_input(shape, fmt, mvb, use_bn, use_res, seed=100 + i, start=i * numel, finite_only=True)
        mn, mx = oracle.c_minmax(ec.expected_t(case, act), False)
        assert np.isfinite(mn).all() and np.isfinite(mx).all()
        batches.append((case, mn, mx))

    def run(case, cur=None, **kw):
        bn = tuple(dev(b) for b in case["bn"]) if use_bn else None
        res = dev(case["res"]) if use_res else None
        return ops.affine_act_minmax(dev(case["x"]), *(cur or ()), bn=bn, residual=res, act=act, **kw)

    for case, mn, mx in batches:                                            # mode 0: the batch's own range
        check_range(run(case), mn, mx, (shape, flags, "current"))
    for mode, momentum in ((1, 0.9), (2, 0.9), (2, 0.5)):
        cur, ref = None, None
        for step, (case, mn, mx) in enumerate(batches):
            packed = dev(np.zeros((1, 4), np.float32))
            got = run(case, cur, mode=mode, momentum=momentum, packed=packed)
            ref = oracle.c_fold(ref[0], ref[1], mn, mx, mode, momentum) if ref else oracle.c_fold(mn, mx, mn, mx, mode, momentum, True)
            gmn, gmx = check_range(got, ref[0], ref[1], (shape, flags, mode, momentum, step))
            np.testing.assert_array_equal(packed.cpu().numpy(), _expect_packed(gmn, gmx))
            cur = (got[0], got[1])
    # specials: a NaN anywhere makes min and max NaN; +inf and -inf reach max and min (through the activation, as t says)
    case = batches[0][0]
    for plant in ((np.nan,), (np.inf, -np.inf), (np.inf, -np.inf, np.nan)):
        c2 = dict(case, x=case["x"].copy())
        flat = c2["x"].reshape(-1)
        for j, v in enumerate(plant):
            flat[(7 * j + 3) % numel] = v
        mn, mx = oracle.c_minmax(ec.expected_t(c2, act), False)
        assert np.isnan(mn[0]) == bool(np.isnan(plant).any()) and (np.isnan(mn[0]) or mx[0] == np.inf)
        packed = dev(np.zeros((1, 4), np.float32))
        gmn, gmx = check_range(run(c2, packed=packed), mn, mx, (shape, flags, plant))
        np.testing.assert_array_equal(packed.cpu().numpy(), _expect_packed(gmn, gmx))
        # ... and folded into a finite running estimate
        for mode in (1, 2):
            cur = run(batches[1][0])
            ref = oracle.c_fold(batches[1][1], batches[1][2], mn, mx, mode, 0.9)
            check_range(run(c2, (cur[0], cur[1]), mode=mode, momentum=0.9), ref[0], ref[1], (shape, flags, plant, mode))
