"""The half lane on the GPU at every case of tests/h16_cases.py: the route from the REAL pointer's phase first (ops.h16_route), then
the whole output bit for bit -- a NaN matches a NaN, everything else by its bits, the sign of zero included; no tolerance, no
sampled subset.  K1: the float32 output equals oracle.c_quantize on the exactly widened input, the half output equals that result
rounded once by torch.  Outputs live between guard elements at the phase the case names; inputs are checked unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import h16_cases as hc
import oracle

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 7.0
TD = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


@pytest.fixture(scope="module")
def ops():
    from fp8q import ops as o
    assert torch.cuda.is_available()
    return o


def _groups():
    from fp8q import ops as o
    return hc.k1_groups(o)


K1 = _groups()


def _same_nan(a, b):
    """a, b CPU tensors of one dtype: NaN at the same places, equal bits elsewhere"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if not torch.equal(a.isnan(), b.isnan()):
        return False
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    a, b = a.nan_to_num(0.0).contiguous(), b.nan_to_num(0.0).contiguous()
    return torch.equal(a.view(it), b.view(it))


def _half(u, dt):
    """uint16 patterns -> CPU tensor of the half type"""
    return torch.from_numpy(np.ascontiguousarray(u).view(np.int16)).view(TD[dt])


def _window(n, dtype, phase):
    """(buffer, an n-element window that starts `phase` elements behind a 16-byte boundary, its offset): GUARD sentinels and more
    on both sides"""
    es = torch.empty(0, dtype=dtype).element_size()
    per = 16 // es
    buf = torch.full((n + 2 * GUARD + 2 * per,), SENTINEL, dtype=dtype, device="cuda")
    off = GUARD + (phase - (buf.data_ptr() // es + GUARD)) % per
    win = buf[off:off + n]
    assert win.data_ptr() % 16 == es * phase
    return buf, win, off


def _guards_intact(buf, off, n):
    c = buf.cpu()
    return bool((c[:off] == SENTINEL).all()) and bool((c[off + n:] == SENTINEL).all())


def _oracle(case, fmt, dt):
    w = hc.widen(case["x"].reshape(-1), dt).reshape(case["x"].shape)
    return torch.from_numpy(oracle.c_quantize(w, case["maxval"], *fmt))


def _run_k1(ops, key, want, case, ref, xd, y_phases):
    """K1 of one key on the device tensor xd (at the key's phase) into guarded windows at the given (dtype, phase) pairs"""
    _, dt, C, inner, fmt, pc, xp = key
    n = C * inner
    assert xd.data_ptr() % 16 == 2 * xp
    got = ops.h16_route("quantize", C, inner, pc, *fmt, x_mod16=xd.data_ptr() % 16)
    assert all(got[f] == v for f, v in want.items()) and not got["nontemporal"], (key, want, got)
    mv = torch.from_numpy(case["maxval"]).cuda()
    for odt, yp in y_phases:
        ybuf, y, yoff = _window(n, odt, yp)
        out = ops.quantize(xd.view(C, inner), mv, *fmt, out=y.view(C, inner))
        assert out.data_ptr() == y.data_ptr()
        assert _same_nan(y.cpu().view(C, inner), ref.to(odt)), (key, odt, yp)
        assert _guards_intact(ybuf, yoff, n), (key, odt, yp)
    assert torch.equal(xd.cpu().view(torch.int16), _half(case["x"].reshape(-1), dt).view(torch.int16)), key


@pytest.mark.parametrize("name", sorted(K1))
def test_k1_reaches_its_kernel_and_matches_the_oracle(ops, name):
    for key, want in K1[name].items():
        _, dt, C, inner, fmt, pc, xp = key
        case = hc.quant_input(key)
        ref = _oracle(case, fmt, dt)
        xbuf, xd, xoff = _window(C * inner, TD[dt], xp)
        xd.copy_(_half(case["x"].reshape(-1), dt))
        _run_k1(ops, key, want, case, ref, xd, [(torch.float32, (xp + 1) % 4), (TD[dt], (3 * xp + 1) % 8)])


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_k1_at_every_x_and_y_phase_and_in_place(ops, dt):
    """views base[i:] for i = 0..7 against every phase of a half output (0..7) and of a float32 output (0..3), then y = x"""
    for base in hc.phase_keys(dt):
        for xp in range(8):
            key = hc.with_phase(base, xp)
            _, _, C, inner, fmt, pc, _ = key
            case = hc.quant_input(key)
            ref = _oracle(case, fmt, dt)
            xbuf, xd, xoff = _window(C * inner, TD[dt], xp)
            xd.copy_(_half(case["x"].reshape(-1), dt))
            want = dict(kernel="k_h16_quant", u=1, head=(8 - xp) % 8)
            _run_k1(ops, key, want, case, ref, xd, [(TD[dt], yp) for yp in range(8)] + [(torch.float32, yp) for yp in range(4)])
            mv = torch.from_numpy(case["maxval"]).cuda()
            out = ops.quantize(xd.view(C, inner), mv, *fmt, out=xd.view(C, inner))
            assert out.data_ptr() == xd.data_ptr()
            assert _same_nan(xd.cpu().view(C, inner), ref.to(TD[dt])), (key, "in place")
            assert _guards_intact(xbuf, xoff, C * inner), (key, "in place")


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_small_tensors_in_place_at_every_phase(ops, dt):
    """tensors of 1..7 and of 77..84 elements quantized onto themselves: heads without a body, every tail"""
    for key, want in K1["tails-%s" % dt].items():
        _, _, C, inner, fmt, pc, xp = key
        case = hc.quant_input(key)
        ref = _oracle(case, fmt, dt)
        xbuf, xd, xoff = _window(C * inner, TD[dt], xp)
        xd.copy_(_half(case["x"].reshape(-1), dt))
        ops.quantize(xd.view(C, inner), torch.from_numpy(case["maxval"]).cuda(), *fmt, out=xd.view(C, inner))
        assert _same_nan(xd.cpu().view(C, inner), ref.to(TD[dt])), key
        assert _guards_intact(xbuf, xoff, C * inner), key


# ---------------------------------------------------------------------------------------------------------------------------
# every bit pattern through every path
# ---------------------------------------------------------------------------------------------------------------------------
PATTERN_SHAPES = [(65536, 9, hc.E4M3, "k_h16_quant"), (65536 * 3 // 8, 24, hc.E5M2, "k_h16_quant"), (65536, 7, hc.E5M2, "k_h16_quant_rows")]


@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("C,inner,fmt,kernel", PATTERN_SHAPES, ids=lambda v: str(v) if isinstance(v, (int, str)) else "")
def test_every_pattern_per_channel(ops, dt, C, inner, fmt, kernel):
    """the 65536 patterns tiled with a rotation per tile: through the straddling groups of 9- and 24-element rows and through the
    row kernel, the rows' ranges cycling through every range of the format; float32 and half out"""
    from epilogue_cases import ranges
    x = hc.all_patterns(C, inner)
    assert x.size % 65536 == 0 and np.array_equal(np.sort(x.reshape(-1)[:65536]), np.arange(65536))
    R = ranges(fmt)
    mvh = np.array([R[r % len(R)] for r in range(C)], np.float32)
    ref = torch.from_numpy(oracle.c_quantize(hc.widen(x.reshape(-1), dt).reshape(C, inner), mvh, *fmt))
    xbuf, xd, _ = _window(C * inner, TD[dt], 0)
    xd.copy_(_half(x.reshape(-1), dt))
    got = ops.h16_route("quantize", C, inner, True, *fmt, x_mod16=xd.data_ptr() % 16)
    assert got["kernel"] == kernel and not got["nontemporal"], got
    mv = torch.from_numpy(mvh).cuda()
    for odt in (torch.float32, TD[dt]):
        ybuf, y, yoff = _window(C * inner, odt, 1)
        ops.quantize(xd.view(C, inner), mv, *fmt, out=y.view(C, inner))
        assert _same_nan(y.cpu().view(C, inner), ref.to(odt)), (dt, C, inner, odt)
        assert _guards_intact(ybuf, yoff, C * inner)


@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("n,C,inner,fmt", [(7, 1, 7, hc.E5M2), (14, 1, 14, hc.E4M3), (14, 2, 7, hc.E5M2), (7, 7, 1, hc.E4M3), (16, 2, 8, hc.E4M3)],
                         ids=lambda v: str(v) if isinstance(v, int) else "")
def test_every_pattern_through_the_scalar_head_and_tail(ops, dt, n, C, inner, fmt):
    """windows of n elements one element behind a 16-byte boundary, the 65536 patterns dealt over them: C = 1 is the per-tensor
    call (7 head scalars, then 7 tail scalars, no group), [2, 7] and [7, 1] the per-channel calls on the same windows (the row
    kernel's scalars), [2, 8] the per-channel chunk kernel with head 7, one straddling group and a tail of 1.  The C entry itself:
    thousands of launches into one buffer, one comparison.  The half result is the float32 result rounded once -- a multiply fused
    with the conversion would round the exact product instead and differ on the ties of the float32 result."""
    from fp8q._lib import check, lib
    L = lib()
    stride = 24
    nwin = -(-65536 // n)
    pat = (np.arange(nwin * n, dtype=np.int64) & 0xffff).astype(np.uint16).reshape(nwin, n)
    pc = C > 1
    rng = [hc.default_maxval(fmt), 0.7361][:C] if pc and C == 2 else ([hc.default_maxval(fmt)] * C if pc else [hc.default_maxval(fmt)])
    mvh = np.array(rng, np.float32)
    mv = torch.from_numpy(mvh).cuda()
    w = hc.widen(pat.reshape(-1), dt).reshape(nwin * C, inner)
    ref = torch.from_numpy(oracle.c_quantize(w, np.tile(mvh, nwin) if pc else mvh, *fmt)).view(nwin, n)
    xbuf, xd, _ = _window(nwin * stride, TD[dt], 1)
    xs = xd.view(nwin, stride)
    xs[:, :n] = _half(pat.reshape(-1), dt).view(nwin, n).cuda()
    got = ops.h16_route("quantize", C, inner, pc, *fmt, x_mod16=xs[5].data_ptr() % 16)
    assert xs[5].data_ptr() % 16 == 2 and got["kernel"] == ("k_h16_quant" if inner >= 8 or not pc else "k_h16_quant_rows"), got
    if got["kernel"] == "k_h16_quant":
        assert (got["head"], got["groups"], got["tail"]) == (min(7, n), max(0, n - 7) // 8, max(0, n - 7) % 8), got
    st = torch.cuda.current_stream().cuda_stream
    for odt in (torch.float32, TD[dt]):
        es = 4 if odt == torch.float32 else 2
        ybuf, yd, yoff = _window(nwin * stride, odt, 1)
        xp, yp = xd.data_ptr(), yd.data_ptr()
        for j in range(nwin):
            rc = L.fp8q_quantize_h16(xp + 2 * stride * j, yp + es * stride * j, DT_CODE[TD[dt]], DT_CODE[odt], C, inner, mv.data_ptr(),
                                     C if pc else 1, float(fmt[0]), fmt[1], fmt[2], st)
            if rc:
                check(rc, "fp8q_quantize_h16")
        y = yd.cpu().view(nwin, stride)
        assert _same_nan(y[:, :n].contiguous(), ref.to(odt)), (dt, n, C, odt)
        assert bool((y[:, n:] == SENTINEL).all()) and _guards_intact(ybuf, yoff, nwin * stride)


# ---------------------------------------------------------------------------------------------------------------------------
# min/max
# ---------------------------------------------------------------------------------------------------------------------------
def _mm_keys():
    from fp8q import ops as o
    return sorted(hc.minmax_keys(o).items(), key=lambda kv: repr(kv[0]))


@pytest.mark.parametrize("key,want", _mm_keys(), ids=lambda v: "-".join(str(e) for e in v[1:]) if isinstance(v, tuple) else "")
def test_minmax_reaches_its_kernel_and_folds_like_the_fp32_entry_and_the_oracle(ops, key, want):
    _, dt, C, inner, xp = key
    batches = [hc.rows_input(dt, C, inner, hc.E4M3, "minmax", seed)[0] for seed in (0, 1)]
    wide = [hc.widen(b.reshape(-1), dt).reshape(C, inner) for b in batches]
    _, xd, _ = _window(C * inner, TD[dt], xp)
    got = ops.h16_route("minmax", C, inner, x_mod16=xd.data_ptr() % 16)
    assert all(got[f] == v for f, v in want.items()) and not got["nontemporal"] and got["launches"] == 1, (key, want, got)
    for mode in (ops.FOLD_CURRENT, ops.FOLD_ALL, ops.FOLD_RUNNING):
        eh = ef = (None, None)
        rmn = rmx = None
        for b, xb in enumerate(batches):
            xd.copy_(_half(xb.reshape(-1), dt))
            rh = ops.minmax(xd.view(C, inner), True, eh[0], eh[1], mode=mode, momentum=0.9, want_maxval=True)
            rf = ops.minmax(torch.from_numpy(wide[b]).cuda(), True, ef[0], ef[1], mode=mode, momentum=0.9, want_maxval=True)
            bmn, bmx = oracle.c_minmax(wide[b], True)
            rmn, rmx = oracle.c_fold(bmn if b == 0 else rmn, bmx if b == 0 else rmx, bmn, bmx, mode, 0.9, first=b == 0)
            refs = (rmn, rmx, oracle.c_absmax(rmn, rmx))
            for a, c, r in zip(rh, rf, refs):
                assert a.dtype == torch.float32
                assert _same_nan(a.cpu(), c.cpu()), (key, mode, b)
                assert _same_nan(a.cpu(), torch.from_numpy(r)), (key, mode, b)
            eh, ef = rh[:2], rf[:2]
    ops.check_workspaces()


def test_minmax_across_the_slab_border(ops):
    """65535 + 3 rows of the streaming kernel: the second launch reads x + 65535 * inner and writes the estimates from row 65535 on"""
    x = hc.slab_input()
    C, inner = x.shape
    got = ops.h16_route("minmax", C, inner)
    assert (got["kernel"], got["launches"], got["grid_y"]) == ("k_h16_minmax_part", 2, hc.SLAB), got
    xt = _half(x.reshape(-1), "bfloat16").view(C, inner)
    want_mn, want_mx = torch.amin(xt, 1).float(), torch.amax(xt, 1).float()
    mn, mx, mv = ops.minmax(xt.cuda(), True, mode=ops.FOLD_CURRENT, want_maxval=True)
    assert _same_nan(mn.cpu(), want_mn) and _same_nan(mx.cpu(), want_mx)
    assert _same_nan(mv.cpu(), torch.maximum(want_mn.abs(), want_mx.abs()))
    rows = slice(hc.SLAB - 1, hc.SLAB + 2)
    assert float(mx[hc.SLAB - 1]) > 3e38 and float(mn[hc.SLAB]) < -3e38 and bool(mn[hc.SLAB + 1].isnan()) and bool(mx[rows].isnan().sum() == 1)
    ops.check_workspaces()


# ---------------------------------------------------------------------------------------------------------------------------
# fused
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", hc.DTYPES)
def test_fused_matches_the_fp32_entry_and_the_oracle_on_its_own_ranges(ops, dt):
    for key, want in hc.fused_keys(ops).items():
        _, kdt, C, inner, fmt, xp = key
        if kdt != dt:
            continue
        xh, kinds = hc.rows_input(dt, C, inner, fmt, "minmax_quantize")
        wide = hc.widen(xh.reshape(-1), dt).reshape(C, inner)
        if C >= 16:
            assert {"nan", "+inf", "-inf", "+0", "-0", "mixed0", "positive", "negative", "denormal"} <= {k for k, _ in kinds}, key
        xbuf, xd, xoff = _window(C * inner, TD[dt], xp)
        xd.copy_(_half(xh.reshape(-1), dt))
        got = ops.h16_route("minmax_quantize", C, inner, True, *fmt, x_mod16=xd.data_ptr() % 16)["stages"]
        assert len(got) == 2 and all(g[f] == v for g, w in zip(got, want) for f, v in w.items()), (key, want, got)
        rmn, rmx = oracle.c_minmax(wide, True)
        rmv = oracle.c_absmax(rmn, rmx)
        ref = torch.from_numpy(oracle.c_quantize(wide, rmv, *fmt))
        yf, mnf, mxf, mvf = ops.minmax_quantize(torch.from_numpy(wide).cuda(), *fmt)
        assert _same_nan(yf.cpu(), ref), key
        for odt, yp in ((torch.float32, (xp + 2) % 4), (TD[dt], (xp + 5) % 8)):
            ybuf, y, yoff = _window(C * inner, odt, yp)
            out, mn, mx, mv = ops.minmax_quantize(xd.view(C, inner), *fmt, out=y.view(C, inner))
            assert out.data_ptr() == y.data_ptr()
            for a, c, r in ((mn, mnf, rmn), (mx, mxf, rmx), (mv, mvf, rmv)):
                assert _same_nan(a.cpu(), c.cpu()) and _same_nan(a.cpu(), torch.from_numpy(r)), (key, odt)
            assert _same_nan(y.cpu().view(C, inner), ref.to(odt)), (key, odt)
            assert _guards_intact(ybuf, yoff, C * inner), (key, odt)
        assert torch.equal(xd.cpu().view(torch.int16), _half(xh.reshape(-1), dt).view(torch.int16)), key
        # in place (half out)
        out, mn, mx, mv = ops.minmax_quantize(xd.view(C, inner), *fmt, out=xd.view(C, inner))
        assert _same_nan(xd.cpu().view(C, inner), ref.to(TD[dt])) and _same_nan(mv.cpu(), torch.from_numpy(rmv)), (key, "in place")
        assert _guards_intact(xbuf, xoff, C * inner), key
