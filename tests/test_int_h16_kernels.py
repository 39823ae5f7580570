"""The uniform (INT) quantizers on float16 / bfloat16 tensors (csrc/fp8q_inth16.hip) against the float32 kernels: the
expected value of every call is fp8q.ops.int_quantize on x.float() (float32 output), and .to(dtype) of that for an output in
x's dtype.  Equality is on bit patterns, a NaN matches any NaN.  Comparisons run on the device: one flag per case comes back."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
PT_SHAPES = [(1,), (33,), (2, 70001), (4, 16, 14, 14)]
PC_SHAPES = [(64, 3, 7, 7), (7, 13, 3), (1, 5), (3, 1, 1), (3000, 1), (5, 4099), (1000, 512)]
NBITS = [2, 4, 8, 16]


def _same(a, b):
    """equal bit patterns, except that a NaN matches any NaN"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = a.isnan(), b.isnan()
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return bool(torch.equal(na, nb)
                and torch.equal(a.masked_fill(na, 0).contiguous().view(it), b.masked_fill(nb, 0).contiguous().view(it)))


def _specials(dtype):
    fi = torch.finfo(dtype)
    return torch.tensor([0.0, -0.0, fi.smallest_normal * fi.eps, -fi.smallest_normal * fi.eps, fi.max, -fi.max, float("inf"),
                         float("-inf"), float("nan")], dtype=torch.float64).to(dtype)


def _data(shape, dtype, seed=0):
    """normals x 3 with the type's special values scattered over the tensor (every row of a short-row shape gets some)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 3).to(dtype).reshape(-1)
    sp = _specials(dtype)
    n = x.numel()
    if n >= 4 * sp.numel():
        pos = (torch.arange(sp.numel()) * (n // sp.numel()) + torch.arange(sp.numel())) % n
        x[pos] = sp
    elif n > 1:
        x[-1] = sp[(seed + n) % sp.numel()]
    return x.reshape(shape).cuda()


def _ranges(C, symmetric, n_bits, seed=0):
    """fixed (x_min, x_max) per channel, turned into (delta, zero_float, signed) by the float32 range kernel"""
    from fp8q import ops
    c = torch.arange(C, dtype=torch.float32, device="cuda")
    x_min = -(2.5 + 0.37 * ((c + seed) % 11))
    x_max = 3.0 + 0.21 * ((c * 7 + seed) % 13)
    return ops.int_set_range(x_min, x_max, n_bits, symmetric)


def _check_fixed(x, d, z, sg, n_bits, symmetric):
    from fp8q import ops
    want = ops.int_quantize(x.float(), d, z, sg, n_bits, symmetric)
    y32 = ops.int_quantize(x, d, z, sg, n_bits, symmetric)
    assert y32.dtype == torch.float32 and _same(y32, want)
    yh = ops.int_quantize(x, d, z, sg, n_bits, symmetric, out_dtype=x.dtype)
    assert yh.dtype == x.dtype and _same(yh, want.to(x.dtype))


@pytest.mark.parametrize("n_bits", NBITS)
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape", PT_SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_per_tensor_matches_fp32_kernel(dtype, shape, symmetric, n_bits):
    x = _data(shape, dtype, seed=n_bits)
    d, z, sg = _ranges(1, symmetric, n_bits)
    _check_fixed(x, d, z, sg, n_bits, symmetric)


@pytest.mark.parametrize("n_bits", NBITS)
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape", PC_SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_per_channel_matches_fp32_kernel(dtype, shape, symmetric, n_bits):
    x = _data(shape, dtype, seed=n_bits)
    d, z, sg = _ranges(shape[0], symmetric, n_bits, seed=3)
    _check_fixed(x, d, z, sg, n_bits, symmetric)


@pytest.mark.parametrize("n_bits", [4, 8])
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_degenerate_positive_minimum_and_non_negative_ranges(dtype, symmetric, n_bits):
    """a channel with x_min == x_max == 0 (scale = eps), one whose minimum is positive (the range still contains 0), and,
    all minima being >= 0, a symmetric quantizer that comes out unsigned"""
    from fp8q import ops
    x = _data((5, 37), dtype, seed=5)
    x_min = torch.tensor([0.0, 0.5, 0.0, 1e-3, 0.25], device="cuda")
    x_max = torch.tensor([0.0, 2.0, 3.0, 7.0, 0.25], device="cuda")
    d, z, sg = ops.int_set_range(x_min, x_max, n_bits, symmetric)
    if symmetric:
        assert not bool(sg)
    _check_fixed(x, d, z, sg, n_bits, symmetric)
    for odt in (torch.float32, dtype):
        y, d2, z2, sg2 = ops.int_range_quantize(x, x_min, x_max, n_bits, symmetric, out_dtype=odt)
        assert _same(y, ops.int_quantize(x.float(), d, z, sg, n_bits, symmetric).to(odt))
        assert _same(d2, d) and (symmetric or _same(z2, z)) and (not symmetric or bool(sg2) == bool(sg))
    # per tensor, non-negative
    d, z, sg = ops.int_set_range(x_min[1:2], x_max[1:2], n_bits, symmetric)
    _check_fixed(x, d, z, sg, n_bits, symmetric)


@pytest.mark.parametrize("n_bits", NBITS)
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_exact_ties(dtype, symmetric, n_bits):
    """x = (k + 0.5) * delta for power-of-two deltas, kept where the half type holds it exactly: rint's half-to-even"""
    from fp8q import ops
    k = torch.arange(-300, 300, dtype=torch.float32) + 0.5
    deltas = [0.25, 2.0 ** -6, 8.0]
    rows = []
    for dl in deltas:
        t = k * dl
        keep = t.to(dtype).float() == t
        assert int(keep.sum()) >= 128
        sel = t[keep]
        rows.append(sel[sel.numel() // 2 - 64:sel.numel() // 2 + 64])        # around zero, both signs
    x = torch.stack(rows).to(dtype).cuda()
    d = torch.tensor(deltas, device="cuda")
    z = None if symmetric else torch.tensor([3.0, 0.5, 1.5], device="cuda")     # 0.5, 1.5: ties of the zero point itself
    sg = torch.ones((), dtype=torch.bool, device="cuda") if symmetric else None
    _check_fixed(x, d, z, sg, n_bits, symmetric)
    _check_fixed(x[0], d[:1], None if symmetric else z[:1], sg, n_bits, symmetric)


@pytest.mark.parametrize("n_bits", [8, 16])
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_every_bit_pattern(dtype, symmetric, n_bits):
    """all 65536 values of the type, per tensor and over 4 channels: a range beyond the type's largest finite value (fp16: the
    fp32 result overflows to infinity when it is narrowed) and ranges inside it (the product scale * (t - zp) is rounded to
    fp32 first, then to the half type: a fused single rounding differs on some of these patterns)"""
    from fp8q import ops
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype).cuda()
    for lo, hi in ((-70000.0, 70000.0), (-1.3, 2.1)):
        d, z, sg = ops.int_set_range(torch.tensor([lo], device="cuda"), torch.tensor([hi], device="cuda"), n_bits, symmetric)
        _check_fixed(x, d, z, sg, n_bits, symmetric)
    x4 = x.view(4, 16384)[:, torch.randperm(16384, generator=torch.Generator().manual_seed(1)).cuda()].contiguous()
    x_min = torch.tensor([-70000.0, -1.3, 0.0, -300.0], device="cuda")
    x_max = torch.tensor([70000.0, 2.1, 0.01, 5.0], device="cuda")
    d, z, sg = ops.int_set_range(x_min, x_max, n_bits, symmetric)
    _check_fixed(x4, d, z, sg, n_bits, symmetric)
    _check_fixed(x4.t().contiguous().view(4, 16384), d, z, sg, n_bits, symmetric)   # every pattern in every channel's mix
    if dtype == torch.float16:
        y = ops.int_quantize(x, *ops.int_set_range(x_min[:1], x_max[:1], n_bits, symmetric), n_bits, symmetric, out_dtype=dtype)
        assert bool(y.isinf().any())                                               # the overflow case is in the data


@pytest.mark.parametrize("pc", [False, True], ids=["pt", "pc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_any_element_offset_and_output_phase(dtype, pc):
    """x starting 1..7 elements behind a 16-byte boundary, y at another phase, equals the aligned call"""
    from fp8q import ops
    shape = (7, 1171) if pc else (8205,)
    n = 7 * 1171 if pc else 8205
    base = _data((n,), dtype, seed=9)
    for symmetric in (True, False):
        d, z, sg = _ranges(shape[0] if pc else 1, symmetric, 8)
        want32 = ops.int_quantize(base.view(shape), d, z, sg, 8, symmetric)
        wanth = ops.int_quantize(base.view(shape), d, z, sg, 8, symmetric, out_dtype=dtype)
        assert _same(want32, ops.int_quantize(base.float().view(shape), d, z, sg, 8, symmetric))
        for o in range(1, 8):
            xb = torch.zeros(n + 16, dtype=dtype, device="cuda")
            assert xb.data_ptr() % 16 == 0
            x = xb[o:o + n].view(shape)
            x.copy_(base.view(shape))
            yb32 = torch.full((n + 16,), 7.0, dtype=torch.float32, device="cuda")
            ybh = torch.full((n + 16,), 7.0, dtype=dtype, device="cuda")
            p32, ph = (o + 1) % 4 + (0 if o % 2 else 1), (o + 3) % 8
            y32 = ops.int_quantize(x, d, z, sg, 8, symmetric, out=yb32[p32:p32 + n].view(shape))
            yh = ops.int_quantize(x, d, z, sg, 8, symmetric, out=ybh[ph:ph + n].view(shape))
            assert _same(y32, want32) and _same(yh, wanth), (o, symmetric)
            # nothing outside the n elements is written, x is not touched
            assert bool((yb32[:p32] == 7).all() and (yb32[p32 + n:] == 7).all())
            assert bool((ybh[:ph] == 7).all() and (ybh[ph + n:] == 7).all())
            assert bool((xb[:o] == 0).all() and (xb[o + n:] == 0).all()) and _same(x, base.view(shape))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_in_place_and_dense_non_contiguous(dtype):
    from fp8q import ops
    for shape, pc in (((9000,), False), ((11, 1023), True)):
        x = _data(shape, dtype, seed=2)
        d, z, sg = _ranges(shape[0] if pc else 1, False, 8)
        want = ops.int_quantize(x.float(), d, z, None, 8, False).to(dtype)
        xb = torch.zeros(x.numel() + 8, dtype=dtype, device="cuda")
        xi = xb[3:3 + x.numel()].view(shape)
        xi.copy_(x)
        y = ops.int_quantize(xi, d, z, None, 8, False, out=xi)
        assert y.data_ptr() == xi.data_ptr() and _same(xi, want)
    # a dense non-contiguous per-tensor input: the storage as it lies, the result keeps x's strides
    x = _data((4, 6, 5, 7), dtype, seed=4).contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous()
    d, z, sg = _ranges(1, True, 8)
    for odt in (torch.float32, dtype):
        y = ops.int_quantize(x, d, None, sg, 8, True, out_dtype=odt)
        assert y.stride() == x.stride() and y.dtype == odt
        assert _same(y.contiguous(), ops.int_quantize(x.float().contiguous(), d, None, sg, 8, True).to(odt))


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape,pc", [((2, 70001), False), ((64, 3, 7, 7), True), ((3000, 1), True), ((5, 4099), True),
                                      ((7, 13, 3), True)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_range_quantize_writes_the_fp32_range(dtype, shape, pc, symmetric):
    """int_range_quantize on half x: delta / zero_float / sign bit-equal to int_set_range, y to the fixed-range kernel.
    (3000, 1) symmetric: more than 2048 channels, the sign comes from the separate kernel."""
    from fp8q import ops
    x = _data(shape, dtype, seed=6)
    C = shape[0] if pc else 1
    xf = x.float().reshape(C, -1)
    fin = torch.where(torch.isfinite(xf), xf, torch.zeros_like(xf))
    x_min, x_max = fin.amin(dim=1), fin.amax(dim=1)
    for n_bits in (4, 8, 16):
        d, z, sg = ops.int_set_range(x_min, x_max, n_bits, symmetric)
        want = ops.int_quantize(x.float(), d, z, sg, n_bits, symmetric)
        for odt in (torch.float32, dtype):
            y, d2, z2, sg2 = ops.int_range_quantize(x, x_min, x_max, n_bits, symmetric, out_dtype=odt)
            assert y.dtype == odt and _same(y, want.to(odt))
            assert d2.dtype == torch.float32 and _same(d2, d)
            if symmetric:
                assert z2 is None and sg2.dtype == torch.bool and bool(sg2) == bool(sg)
            else:
                assert _same(z2, z)
    if symmetric and pc:     # a non-negative vector and a NaN in it: unsigned both times, as int_set_range
        for xm in (x_min.abs(), torch.where(torch.arange(C, device="cuda") == C // 2, float("nan"), x_min)):
            d, z, sg = ops.int_set_range(xm, x_max, 8, True)
            y, d2, _, sg2 = ops.int_range_quantize(x, xm, x_max, 8, True, out_dtype=dtype)
            assert not bool(sg2) and not bool(sg) and _same(d2, d)
            assert _same(y, ops.int_quantize(x.float(), d, None, sg, 8, True).to(dtype))


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape", [(64, 3, 7, 7), (3000, 1), (5, 4099), (3, 5000), (1, 5)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_minmax_quantize_matches_the_fp32_twin(dtype, shape, symmetric):
    """row min / max bit-equal to int_minmax_quantize on x.float() (rows with a NaN included), the ranges and y with them"""
    from fp8q import ops
    x = _data(shape, dtype, seed=8)                  # NaN and +-inf in some rows
    w = ops.int_minmax_quantize(x.float(), 8, symmetric)
    assert bool(w[1].isnan().any()) or shape[0] == 1
    for odt in (torch.float32, dtype):
        r = ops.int_minmax_quantize(x, 8, symmetric, out_dtype=odt)
        assert r[0].dtype == odt and _same(r[0], w[0].to(odt))
        assert _same(r[1], w[1]) and _same(r[2], w[2]) and _same(r[3], w[3])
        if symmetric:
            assert r[4] is None and bool(r[5]) == bool(w[5])
        else:
            assert _same(r[4], w[4])
    xf = torch.nan_to_num(x.float(), nan=0.5, posinf=3.0, neginf=-3.0).to(dtype)    # finite rows: a signed range
    w = ops.int_minmax_quantize(xf.float(), 8, symmetric)
    r = ops.int_minmax_quantize(xf, 8, symmetric, out_dtype=dtype)
    assert _same(r[0], w[0].to(dtype)) and _same(r[1], w[1]) and _same(r[2], w[2]) and _same(r[3], w[3])
    assert symmetric and bool(r[5]) == bool(w[5]) or not symmetric and _same(r[4], w[4])


def test_nontemporal_variants_past_the_threshold():
    """one bf16 tensor just past 64 MiB: 2^25 + 5 elements per tensor, and rows of 147 covering them per channel, against the
    float32 kernel chain on the device"""
    from fp8q import ops
    dtype = torch.bfloat16
    n = (1 << 25) + 5
    C = -(-n // 147)
    g = torch.Generator(device="cuda").manual_seed(3)
    buf = (torch.randn(C * 147, device="cuda", generator=g) * 3).to(dtype)
    buf[:9] = _specials(dtype).cuda()
    buf[n - 9:n] = _specials(dtype).cuda()
    x = buf[:n]
    assert x.numel() * 2 >= 64 << 20
    for symmetric in (True, False):
        d, z, sg = _ranges(1, symmetric, 8)
        want = ops.int_quantize(x.float(), d, z, sg, 8, symmetric)
        assert _same(ops.int_quantize(x, d, z, sg, 8, symmetric, out_dtype=dtype), want.to(dtype))
        assert _same(ops.int_quantize(x, d, z, sg, 8, symmetric), want)
        del want
    rows = buf.view(C, 147)
    d, z, sg = _ranges(C, False, 8, seed=1)
    want = ops.int_quantize(rows.float(), d, z, None, 8, False)
    assert _same(ops.int_quantize(rows, d, z, None, 8, False, out_dtype=dtype), want.to(dtype))
    assert _same(ops.int_quantize(rows, d, z, None, 8, False), want)
    xm, xx = -(d * 100), d * 155
    y, d2, z2, _ = ops.int_range_quantize(rows, xm, xx, 8, False, out_dtype=dtype)
    d3, z3, _ = ops.int_set_range(xm, xx, 8, False)
    assert _same(d2, d3) and _same(z2, z3)
    assert _same(y, ops.int_quantize(rows.float(), d3, z3, None, 8, False).to(dtype))


# ---- routing ---------------------------------------------------------------------------------------------------------
def _quantizer(symmetric, per_channel, keep_dtype, C=6):
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    cls = SymmetricUniformQuantizer if symmetric else AsymmetricUniformQuantizer
    q = cls(n_bits=8, per_channel=per_channel, keep_dtype=keep_dtype).cuda()
    n = C if per_channel else 1
    c = torch.arange(n, dtype=torch.float32, device="cuda")
    lo, hi = -(1.0 + 0.3 * c), 2.0 + 0.2 * c
    q.set_quant_range(lo if per_channel else lo.reshape(()), hi if per_channel else hi.reshape(()))
    return q


def _raise(*a, **k):
    raise AssertionError("the eager chain ran")


@pytest.mark.parametrize("per_channel", [False, True], ids=["pt", "pc"])
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_keep_dtype_runs_the_half_kernels(dtype, symmetric, per_channel, monkeypatch):
    from fp8q import ops
    q = _quantizer(symmetric, per_channel, True)
    x = _data((6, 50), dtype, seed=1)
    want = ops.int_quantize(x.float(), q._delta, None if symmetric else q._zero_float, q._signed if symmetric else None, 8,
                            symmetric).to(dtype)
    with monkeypatch.context() as m:
        m.setattr(torch, "round", _raise)
        with torch.no_grad():
            y = q(x)
            assert y.dtype == dtype and _same(y, want)
            # range-setting forwards: half kernels too, the ranges written are those of the float32 range kernel
            lo = torch.full((6,) if per_channel else (), -1.5, device="cuda")
            hi = torch.full((6,) if per_channel else (), 2.5, device="cuda")
            y2 = q._range_forward(x, lo, hi)
            d, z, sg = ops.int_set_range(lo, hi, 8, symmetric)
            assert y2.dtype == dtype and _same(q._delta, d)
            assert _same(y2, ops.int_quantize(x.float(), d, z, sg, 8, symmetric).to(dtype))
            if per_channel:
                y3, mn, mx = q._minmax_forward(x)
                w = ops.int_minmax_quantize(x.float(), 8, symmetric)
                assert y3.dtype == dtype and _same(y3, w[0].to(dtype)) and _same(mn, w[1]) and _same(mx, w[2])
                assert _same(q._delta, w[3])
    # under autograd: widened, the float32 route, cast back -- same values, and a gradient arrives in x's dtype
    q = _quantizer(symmetric, per_channel, True)
    xf = torch.nan_to_num(x.float(), nan=0.0, posinf=1.0, neginf=-1.0).to(dtype)
    xg = xf.clone().requires_grad_(True)
    yg = q(xg)
    assert yg.dtype == dtype and yg.requires_grad
    with torch.no_grad():
        assert _same(yg.detach(), q(xf))
    yg.float().sum().backward()
    assert xg.grad is not None and xg.grad.dtype == dtype


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_int_kernels_off_is_the_eager_chain(dtype, monkeypatch):
    q = _quantizer(True, False, True)
    x = _data((6, 50), dtype, seed=1)
    monkeypatch.setenv("FP8Q_INT_KERNELS", "0")
    with monkeypatch.context() as m:
        m.setattr(torch, "round", _raise)
        with torch.no_grad(), pytest.raises(AssertionError, match="eager chain"):
            q(x)
    # keep_dtype=False, called directly: the eager chain as well, kernels on or off
    monkeypatch.delenv("FP8Q_INT_KERNELS")
    q = _quantizer(True, False, False)
    with monkeypatch.context() as m:
        m.setattr(torch, "round", _raise)
        with torch.no_grad(), pytest.raises(AssertionError, match="eager chain"):
            q(x)


@pytest.mark.parametrize("estimating", [False, True], ids=["fixed", "estimating"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["pt", "pc"])
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
def test_manager_keep_dtype_false_is_float32_as_before(symmetric, per_channel, estimating):
    """through the manager without keep_dtype: float32 output, bit-equal to the manager on x.float(); with keep_dtype: x's
    dtype, that result rounded once"""
    from quantization.manager import QuantizationManager
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    qm = QMethods.symmetric_uniform.cls if symmetric else QMethods.asymmetric_uniform.cls

    def make(keep):
        return QuantizationManager(qmethod=qm, init=RangeEstimators.current_minmax.cls, per_channel=per_channel,
                                   qparams=dict(n_bits=8, keep_dtype=keep)).cuda()
    for dtype in DTYPES:
        x = torch.nan_to_num(_data((6, 50), dtype, seed=12).float(), nan=0.25, posinf=2.0, neginf=-2.0).to(dtype)
        a, b, k = make(False), make(False), make(True)
        with torch.no_grad():
            for m, inp in ((a, x), (b, x.float()), (k, x)):
                m(inp)
                if not estimating:
                    m.fix_ranges()
            ya, yb, yk = a(x), b(x.float()), k(x)
        assert ya.dtype == torch.float32 and _same(ya, yb)
        assert yk.dtype == dtype and _same(yk, yb.to(dtype))
        for m in (a, k):
            assert _same(m.quantizer._delta, b.quantizer._delta) and m.quantizer._delta.dtype == torch.float32
            if not symmetric:
                assert _same(m.quantizer._zero_float, b.quantizer._zero_float)
