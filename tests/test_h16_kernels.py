"""The half-precision lane on the GPU (csrc/fp8q_h16.hip): fp16 / bf16 inputs give, bit for bit, what the fp32
contract gives on the exactly widened input -- the oracle for K1, the fp32 entry points for min/max -- and a half output
is that result rounded once by torch.  Equality means equal bit patterns, except that a NaN matches any NaN."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
FORMATS = ((8, 2, 1), (8, 3, 1), (8, 4, 1), (8, 3, 0), (6, 2, 1))       # (n_bits, M, sign_bits)
GUARD = 64


def _ops():
    from fp8q import ops
    return ops


def _same_nan(a, b):
    """a, b CPU tensors of one dtype: NaN at the same places, equal bits elsewhere"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if not torch.equal(a.isnan(), b.isnan()):
        return False
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    a, b = a.nan_to_num(0.0).contiguous(), b.nan_to_num(0.0).contiguous()
    return torch.equal(a.view(it), b.view(it))


def _oracle(xf, mv, fmt):
    """the fp32 contract on an fp32 CPU tensor"""
    n_bits, M, s = fmt
    return torch.from_numpy(oracle.c_quantize(xf.numpy(), mv.numpy(), float(M), n_bits, s))


def _guarded(n, dtype, device):
    """(whole buffer, the n-element window behind GUARD sentinel elements)"""
    buf = torch.full((n + 2 * GUARD,), 7.0, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    c = buf.cpu()
    return bool((c[:GUARD] == 7.0).all()) and bool((c[GUARD + n:] == 7.0).all())


def _all_patterns(dtype):
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_inputs(dtype):
    """every bit pattern of the input type, every format, five ranges: fp32 out == oracle(widen(x)), half out == that .to(dtype)"""
    ops = _ops()
    x = _all_patterns(dtype)
    xf = x.float()
    xd = x.cuda()
    bad = []
    for fmt in FORMATS:
        n_bits, M, s = fmt
        for mval in (0.37, 1.0, 448.0, 3e-5, 6e4):
            mv = torch.tensor([mval], dtype=torch.float32)
            want = _oracle(xf, mv, fmt)
            got = ops.quantize(xd, mv.cuda(), float(M), n_bits, s)
            assert got.dtype == torch.float32
            if not _same_nan(got.cpu(), want):
                bad.append((fmt, mval, "f32", int((got.cpu().view(torch.int32) != want.view(torch.int32)).sum())))
            got_h = ops.quantize(xd, mv.cuda(), float(M), n_bits, s, out_dtype=dtype)
            assert got_h.dtype == dtype
            if not _same_nan(got_h.cpu(), want.to(dtype)):
                bad.append((fmt, mval, "half", -1))
    assert not bad, bad


def _rand(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp(torch.randn(shape, generator=g))
    return x.to(dtype)


SHAPES = [(C, inner) for inner in (1, 3, 7, 147, 1023, 4097, 65536 + 5) for C in (1, 5, 64, 1000) if C * inner <= 1 << 24]


@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_and_alignment(dtype):
    """per channel and per tensor on [C, inner], contiguous and as the view base[1:] (2-byte aligned start), fp32 and half
    outputs written into guarded buffers"""
    ops = _ops()
    bad = []
    for k, (C, inner) in enumerate(SHAPES):
        fmt = FORMATS[k % len(FORMATS)]
        n_bits, M, s = fmt
        x = _rand((C, inner), dtype, 100 + k)
        xf = x.float()
        mvc = xf.abs().amax(1).clamp_min(1e-3) * 0.75                   # per channel: clips some elements
        mvt = mvc.amax().reshape(1)
        base = torch.zeros(C * inner + 1, dtype=dtype, device="cuda")
        base[1:] = x.reshape(-1).cuda()
        views = (("contig", x.cuda()), ("view", base[1:].view(C, inner)))
        assert views[1][1].data_ptr() % 4 == 2
        for pc, mv in ((True, mvc), (False, mvt)):
            want = _oracle(xf, mv, fmt)
            for vname, xd in views:
                for odt in (torch.float32, dtype):
                    buf, win = _guarded(C * inner, odt, "cuda")
                    y = ops.quantize(xd, mv.cuda(), float(M), n_bits, s, out=win)
                    assert y.data_ptr() == win.data_ptr()
                    ok = _same_nan(win.cpu().view(C, inner), want.to(odt)) and _guards_intact(buf, C * inner)
                    if not ok:
                        bad.append((C, inner, fmt, pc, vname, str(odt)))
    assert not bad, bad


@pytest.mark.parametrize("dtype,pc", [(torch.float16, True), (torch.bfloat16, False)])
def test_streaming_sizes(dtype, pc):
    """tensors beyond the caches (> 64 MiB of half: 16 KiB pieces per block, nontemporal accesses), odd start"""
    ops = _ops()
    C, inner = 228263, 147                                               # 33.5 M elements
    fmt = (8, 2, 1)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(C * inner + 1, generator=g).to(dtype)
    xd = x.cuda()[1:].view(C, inner)
    xf = x[1:].view(C, inner).float()
    mv = xf.abs().amax(1) * 0.9 if pc else torch.tensor([2.5])
    want = _oracle(xf, mv, fmt)
    for odt in (torch.float32, dtype):
        buf, win = _guarded(C * inner, odt, "cuda")
        ops.quantize(xd, mv.cuda(), 2.0, 8, 1, out=win)
        assert _same_nan(win.cpu().view(C, inner), want.to(odt)) and _guards_intact(buf, C * inner), (pc, odt)
        del buf, win


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_and_channels_last(dtype):
    ops = _ops()
    fmt = (8, 3, 1)
    for shape, pc in (((64, 147), True), ((5, 4097), False), ((1000, 7), True)):
        x = _rand(shape, dtype, 7)
        xf = x.float()
        mv = (xf.abs().amax(1) * 0.5 + 1e-3) if pc else torch.tensor([1.5])
        want = _oracle(xf, mv, fmt).to(dtype)
        base = torch.zeros(x.numel() + 1, dtype=dtype, device="cuda")
        base[1:] = x.reshape(-1).cuda()
        xd = base[1:].view(shape)
        y = ops.quantize(xd, mv.cuda(), 3.0, 8, 1, out=xd)              # y aliases x, 2-byte aligned start
        assert y.data_ptr() == xd.data_ptr()
        assert _same_nan(xd.cpu(), want), shape
        assert float(base[0]) == 0.0
    # channels-last activation, per tensor: the storage as it lies, strides kept
    x = _rand((8, 32, 14, 14), dtype, 9).cuda().to(memory_format=torch.channels_last)
    mv = torch.tensor([2.0])
    for odt in (None, dtype):
        y = ops.quantize(x, mv.cuda(), 3.0, 8, 1, out_dtype=odt)
        assert y.stride() == x.stride() and y.dtype == (odt or torch.float32)
        want = _oracle(x.float().cpu().contiguous(), mv, fmt).to(y.dtype)
        assert _same_nan(y.cpu().contiguous(), want)


def _special_rows(dtype):
    """rows with NaN, rows mixing -0.0 and +0.0, an all-zero row of each sign"""
    x = _rand((8, 300), dtype, 21)
    x[1, 17] = float("nan")
    x[2] = 0.0
    x[2, ::2] = -0.0
    x[3] = -0.0
    x[4] = 0.0
    x[5] = x[5].abs()
    x[5, 3] = -0.0
    x[6] = -x[6].abs()
    x[6, 250] = 0.0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
def test_minmax_equals_fp32_entry(dtype):
    """three fold modes over three batches, per tensor and per channel: estimates and maxval bit-equal to the fp32 entry on
    x.float(); NaN rows, signed zeros, odd starts, a split row of 2^22 elements"""
    ops = _ops()
    cases = [("special", lambda b: _special_rows(dtype) * (b + 1)),
             ("short", lambda b: _rand((1000, 7), dtype, 30 + b)),
             ("rows147", lambda b: _rand((64, 147), dtype, 40 + b)),
             ("rows4097", lambda b: _rand((5, 4097), dtype, 50 + b)),
             ("long", lambda b: _rand((3, 65536 + 5), dtype, 60 + b))]
    for name, make in cases:
        for pc in (True, False):
            for mode in (ops.FOLD_CURRENT, ops.FOLD_ALL, ops.FOLD_RUNNING):
                eh = ef = (None, None)
                for b in range(3):
                    x = make(b)
                    base = torch.zeros(x.numel() + 1, dtype=dtype, device="cuda")
                    base[1:] = x.reshape(-1).cuda()
                    xd = base[1:].view(x.shape) if b == 1 else x.cuda()
                    rh = ops.minmax(xd, pc, eh[0], eh[1], mode=mode, momentum=0.9, want_maxval=True)
                    rf = ops.minmax(x.float().cuda(), pc, ef[0], ef[1], mode=mode, momentum=0.9, want_maxval=True)
                    for a, c in zip(rh, rf):
                        assert a.dtype == torch.float32
                        assert _same_nan(a.cpu(), c.cpu()), (name, pc, mode, b)
                    eh, ef = rh[:2], rf[:2]
    x = _rand((1, 1 << 22), dtype, 77)
    x[0, 12345] = -0.0
    rh = ops.minmax(x.cuda(), False, want_maxval=True)
    rf = ops.minmax(x.float().cuda(), False, want_maxval=True)
    for a, c in zip(rh, rf):
        assert _same_nan(a.cpu(), c.cpu())
    assert float(rh[0]) == float(x.float().min()) and float(rh[1]) == float(x.float().max())
    ops.check_workspaces()                                               # raises on a reducer time-out / dirty workspace


WEIGHT_SHAPES = ((64, 3, 7, 7), (512, 512, 3, 3), (32, 1, 3, 3), (1280, 320, 1, 1), (1000, 512))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_minmax_quantize(dtype):
    ops = _ops()
    for k, shape in enumerate(WEIGHT_SHAPES):
        x = (_rand(shape, torch.float32, 80 + k) * 0.05).to(dtype)
        for n_bits, M, s in ((8, 3, 1), (8, 2, 1)):
            yf, mnf, mxf, mvf = ops.minmax_quantize(x.float().cuda(), float(M), n_bits, s)
            y, mn, mx, mv = ops.minmax_quantize(x.cuda(), float(M), n_bits, s)
            assert y.dtype == torch.float32 and y.shape == x.shape
            for a, c in ((y, yf), (mn, mnf), (mx, mxf), (mv, mvf)):
                assert _same_nan(a.cpu(), c.cpu()), (shape, M)
            yh, mn, mx, mv = ops.minmax_quantize(x.cuda(), float(M), n_bits, s, out_dtype=dtype)
            assert yh.dtype == dtype
            assert _same_nan(yh.cpu(), yf.cpu().to(dtype)), (shape, M)
            assert _same_nan(mv.cpu(), mvf.cpu())
            # and the oracle itself
            assert _same_nan(yf.cpu(), _oracle(x.float().reshape(shape[0], -1), mvf.cpu(), (n_bits, M, s)).view(shape))


def test_fp32_dispatch_untouched():
    """fp32 calls give the oracle's bits as before, and have one result dtype"""
    ops = _ops()
    from fp8q._lib import Fp8qError
    x = _rand((64, 147), torch.float32, 5)
    mv = x.abs().amax(1) * 0.5
    y = ops.quantize(x.cuda(), mv.cuda(), 3.0, 8, 1)
    assert y.dtype == torch.float32 and _same_nan(y.cpu(), _oracle(x, mv, (8, 3, 1)))
    mn, mx, mvo = ops.minmax(x.cuda(), True, want_maxval=True)
    omn, omx = oracle.c_minmax(x.numpy(), True)
    assert _same_nan(mn.cpu(), torch.from_numpy(omn)) and _same_nan(mx.cpu(), torch.from_numpy(omx))
    assert _same_nan(mvo.cpu(), torch.from_numpy(oracle.c_absmax(omn, omx)))
    y2, mn2, mx2, mv2 = ops.minmax_quantize(x.cuda(), 3.0, 8, 1)
    assert _same_nan(mv2.cpu(), mvo.cpu())
    assert _same_nan(y2.cpu(), _oracle(x, mv2.cpu(), (8, 3, 1)))
    with pytest.raises(Fp8qError, match="out_dtype"):
        ops.quantize(x.cuda(), mv.cuda(), 3.0, out_dtype=torch.bfloat16)
