"""The row kernels on the GPU at every shape of tests/rows_cases.py: the route from the REAL pointers' phases first
(ops.rows_route), then the whole output against the CPU oracle on integers -- identical NaN masks, identical int32 bits
elsewhere, the sign of zero included; no tolerance, no sampled subset.  Outputs live inside buffers with guard elements before
and after, checked unchanged."""
import numpy as np
import pytest
import torch

import oracle
import rows_cases as rc
from epilogue_cases import same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 7.0


@pytest.fixture(scope="module")
def ops():
    from fp8q import ops as o
    assert torch.cuda.is_available()
    return o


def _keys():
    from fp8q import ops as o
    return sorted(rc.build_shapes(o).items(), key=lambda kv: repr(kv[0]))


KEYS = _keys()


def _window(n, phase):
    """(buffer, an n-element window that starts `phase` elements behind a 16-byte boundary, GUARD sentinels and more around it)"""
    buf = torch.full((n + 2 * GUARD + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    off = GUARD + (phase - (buf.data_ptr() // 4 + GUARD)) % 4
    win = buf[off:off + n]
    assert win.data_ptr() % 16 == 4 * phase
    return buf, win, off


def _guards_intact(buf, off, n):
    c = buf.cpu()
    return bool((c[:off] == SENTINEL).all()) and bool((c[off + n:] == SENTINEL).all())


def _assert_route(ops, key, want, x, y=None):
    op, C, inner, fmt = key[:4]
    got = ops.rows_route(rc.base_op(op), C, inner, rc.pc_of(op), *fmt, x_mod16=x.data_ptr() % 16,
                         y_mod16=(y.data_ptr() % 16) if y is not None else 0, in_place=y is not None and y.data_ptr() == x.data_ptr())
    assert all(got[k] == v for k, v in want.items()), (key, want, got)


@pytest.mark.parametrize("key,want", [kv for kv in KEYS if rc.base_op(kv[0][0]) == "quantize"], ids=lambda v: repr(v) if isinstance(v, tuple) else "")
def test_quantize_reaches_its_kernel_and_matches_the_oracle(ops, key, want):
    op, C, inner, fmt, xp, yp, ip = key
    case = rc.case_input((C, inner), fmt, op)
    n = C * inner
    xbuf, x, xoff = _window(n, xp)
    x.copy_(torch.from_numpy(case["x"].reshape(-1)))
    ybuf, y, yoff = (xbuf, x, xoff) if ip else _window(n, yp)
    _assert_route(ops, key, want, x, y)
    mv = torch.from_numpy(case["maxval"]).cuda()
    ref = oracle.c_quantize(case["x"], case["maxval"], *fmt)
    out = ops.quantize(x.view(C, inner), mv, *fmt, out=y.view(C, inner))
    assert out.data_ptr() == y.data_ptr()
    assert same_bits(y.cpu().numpy().reshape(C, inner), ref), key
    assert _guards_intact(ybuf, yoff, n), key
    if not ip:
        assert np.array_equal(x.cpu().numpy().view(np.int32), case["x"].reshape(-1).view(np.int32))


def _ranges(R):
    """three guarded [R] range vectors (min, max, maxval) in one sentinel-filled buffer"""
    buf = torch.full((3, R + 2 * GUARD), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, [buf[i, GUARD:GUARD + R] for i in range(3)]


def _range_guards_intact(buf, R):
    c = buf.cpu()
    return bool((c[:, :GUARD] == SENTINEL).all()) and bool((c[:, GUARD + R:] == SENTINEL).all())


def _raw_stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("key,want", [kv for kv in KEYS if kv[0][0] == "minmax_quantize"], ids=lambda v: repr(v) if isinstance(v, tuple) else "")
def test_fused_reaches_its_kernel_and_matches_the_oracle(ops, key, want):
    """the C entry itself, so that the range vectors too lie between guard elements"""
    from fp8q._lib import check, lib
    op, C, inner, fmt, xp, yp, ip = key
    case = rc.case_input((C, inner), fmt, op)
    n = C * inner
    xbuf, x, xoff = _window(n, xp)
    x.copy_(torch.from_numpy(case["x"].reshape(-1)))
    ybuf, y, yoff = (xbuf, x, xoff) if ip else _window(n, yp)
    _assert_route(ops, key, want, x, y)
    rmn, rmx = oracle.c_minmax(case["x"], True)
    rmv = oracle.c_absmax(rmn, rmx)
    ref = oracle.c_quantize(case["x"], rmv, *fmt)
    rbuf, (mn, mx, mv) = _ranges(C)
    check(lib().fp8q_minmax_quantize_f32(x.data_ptr(), y.data_ptr(), C, inner, mn.data_ptr(), mx.data_ptr(), mv.data_ptr(),
                                         float(fmt[0]), fmt[1], fmt[2], _raw_stream()), "fp8q_minmax_quantize_f32")
    assert same_bits(mn.cpu().numpy(), rmn) and same_bits(mx.cpu().numpy(), rmx) and same_bits(mv.cpu().numpy(), rmv), key
    assert same_bits(y.cpu().numpy().reshape(C, inner), ref), key
    assert _guards_intact(ybuf, yoff, n) and _range_guards_intact(rbuf, C), key


@pytest.mark.parametrize("key,want", [kv for kv in KEYS if rc.base_op(kv[0][0]) == "minmax"], ids=lambda v: repr(v) if isinstance(v, tuple) else "")
def test_minmax_reaches_its_kernel_and_folds_like_the_oracle(ops, key, want):
    """overwrite, all-min/max and EMA folds over two batches, `first` on and off, with maxval_out: the C entry itself on guarded
    range vectors.  A per-tensor case has finite rows only in its two batches (one NaN would own the result) and a third,
    overwriting call on the batch with a NaN row."""
    from fp8q._lib import check, lib
    op, C, inner, fmt, xp, _, _ = key
    pc = rc.pc_of(op)
    n = C * inner
    batches = [rc.case_input((C, inner), fmt, op, seed)["x"] for seed in (0, 1)]
    _, x, _ = _window(n, xp)
    R, row = (C, inner) if pc else (1, n)
    L = lib()
    wsb = L.fp8q_minmax_workspace_bytes(R, row)
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")           # zero once; every call leaves it zero

    def call(mode, first, vec):
        check(L.fp8q_minmax_f32(x.data_ptr(), R, row, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), mode, 0.9, int(first),
                                ws.data_ptr(), wsb, _raw_stream()), "fp8q_minmax_f32")

    for mode in (ops.FOLD_CURRENT, ops.FOLD_ALL, ops.FOLD_RUNNING):
        rbuf, vec = _ranges(R)
        rmn = rmx = None
        for b, xb in enumerate(batches):
            x.copy_(torch.from_numpy(xb.reshape(-1)))
            _assert_route(ops, key, want, x)
            bmn, bmx = oracle.c_minmax(xb, pc)
            rmn, rmx = oracle.c_fold(bmn if b == 0 else rmn, bmx if b == 0 else rmx, bmn, bmx, mode, 0.9, first=b == 0)
            call(mode, b == 0, vec)
            assert same_bits(vec[0].cpu().numpy(), rmn) and same_bits(vec[1].cpu().numpy(), rmx), (key, mode, b)
            assert same_bits(vec[2].cpu().numpy(), oracle.c_absmax(rmn, rmx)), (key, mode, b)
            assert pc or (np.isfinite(rmn).all() and np.isfinite(rmx).all()), (key, mode, b)
        assert _range_guards_intact(rbuf, R), (key, mode)
    if not pc:
        xb = rc.case_input((C, inner), fmt, op, 0, nan=True)["x"]
        x.copy_(torch.from_numpy(xb.reshape(-1)))
        rbuf, vec = _ranges(1)
        call(ops.FOLD_CURRENT, True, vec)
        assert all(np.isnan(v.cpu().numpy()).all() for v in vec) and np.isnan(oracle.c_minmax(xb, False)[0]).all(), key
        assert _range_guards_intact(rbuf, 1), key
    assert not ws.cpu().numpy().any(), key


# (format, C, inner, x / y phase, in place) -> kernel and, for k_rows_direct, whether it is the instance with tables
TIE_CASES = [
    (rc.E5M2, 120, 147, 0, False, "k_rows_flat", False), (rc.E4M3, 120, 147, 0, False, "k_rows_flat", False),
    (rc.E5M2, 9, 2048, 0, False, "k_quant_rows", False), (rc.E4M3, 9, 2048, 0, False, "k_quant_rows", False),
    (rc.E5M2, 120, 147, 1, False, "k_rows_direct", True), (rc.E4M3, 120, 147, 1, False, "k_rows_direct", True),
    (rc.E5M2, 200, 40, 1, True, "k_rows_direct", False), (rc.E4M3, 200, 40, 1, True, "k_rows_direct", True),
    (rc.E5M2, 2000, 40, 2, False, "k_rows_direct", False), (rc.E4M3, 2000, 40, 2, False, "k_rows_direct", True),
    (rc.E5M2, 300, 4, 0, False, "k_rows_direct", False), (rc.E4M3, 300, 4, 0, False, "k_rows_direct", False),
    # the kernel without tables at three and more mantissa bits, thousands of first-binade elements
    (rc.E4M3, 3000, 30, 1, False, "k_rows_direct", False), (rc.E4M3, 300, 18, 0, False, "k_rows_direct", False),
    (rc.E7, 100, 200, 1, False, "k_rows_direct", False),
]


@pytest.mark.parametrize("fmt,C,inner,xp,ip,kernel,lut", TIE_CASES, ids=lambda v: repr(v) if isinstance(v, tuple) else str(v))
def test_values_next_to_ties_take_the_exact_quotient(ops, fmt, C, inner, xp, ip, kernel, lut):
    """K1 on rows of near-ties at scales that are no power of two: the fast quotient must be redone by division wherever it comes
    close to a tie (quant_group, quant_one), and the kernel without tables must divide in its first binade as in every other.
    (With two mantissa bits the reciprocal quotient never differs from the division on these values: the E4M3 and seven-exponent-
    bit cases are the ones that tell.)"""
    xh, mvh = rc.tie_cloud(fmt, C, inner, C + inner)
    n = C * inner
    xbuf, x, xoff = _window(n, xp)
    x.copy_(torch.from_numpy(xh.reshape(-1)))
    ybuf, y, yoff = (xbuf, x, xoff) if ip else _window(n, xp)
    _assert_route(ops, ("quantize", C, inner, fmt), dict(kernel=kernel, lut=lut), x, y)
    ref = oracle.c_quantize(xh, mvh, *fmt)
    ops.quantize(x.view(C, inner), torch.from_numpy(mvh).cuda(), *fmt, out=y.view(C, inner))
    assert same_bits(y.cpu().numpy().reshape(C, inner), ref), (fmt, C, inner)
    assert _guards_intact(ybuf, yoff, n)
