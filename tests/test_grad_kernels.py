"""The backward kernel (fp8q_quantize_bwd_f32 through fp8q.ops.quantize_backward) against the torch chain of
quantization/fp8.py:_FakeQuantSTE (FP8Q_GRAD_KERNELS=0) on the same device buffers.

  gx                bit-identical everywhere (NaN, +-inf, +-0, denormals, elements on the bounds included);
  gmaxval, gmbits   against a float64 host sum of the SAME fp32 per-element terms (formed in numpy in the chain's order from
                    the HIP forward's y): |difference| <= 2^-22 * sum |term| per row -- fp32 terms exact to the chain's
                    rounding, fp64 accumulation, one final fp32 rounding (2^-24 relative) leave a factor of four to spare.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -22
F32 = np.float32


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _chain(x, g, mv, mb, n_bits, sb, monkeypatch):
    """(y, gx, gmaxval, gmbits) of the torch chain: the parent's backward"""
    from quantization.fp8 import quantize_to_fp8_ste_MM
    monkeypatch.setenv("FP8Q_GRAD_KERNELS", "0")
    xt, mvt = x.clone().requires_grad_(True), mv.clone().requires_grad_(True)
    mbt = torch.tensor([float(mb)], requires_grad=True)
    y = quantize_to_fp8_ste_MM(xt, n_bits, mvt, mbt, sb)
    y.backward(g)
    monkeypatch.delenv("FP8Q_GRAD_KERNELS")
    return y.detach(), xt.grad, mvt.grad, mbt.grad


def _host_sums(x, y, g, mv, sb, per_channel):
    """float64 row sums of the chain's fp32 terms g * w and g * (y - xc), and of their magnitudes"""
    x, y, g, mv = (t.detach().cpu().numpy() for t in (x, y, g, mv))
    C = mv.size if per_channel else 1
    x, y, g = x.reshape(C, -1), y.reshape(C, -1), g.reshape(C, -1)
    m = mv.reshape(C, 1)
    lo = -m if sb == 1 else np.zeros_like(m)
    with np.errstate(all="ignore"):
        xc = np.minimum(np.maximum(x, lo), m)
        d = y - xc
        w = d / m
        w = w + (x > m).astype(F32)
        w = w + F32(0.5) * (x == m).astype(F32)
        if sb == 1:
            w = w - (x < lo).astype(F32)
            w = w - F32(0.5) * (x == lo).astype(F32)
        ta, tb = g * w, g * d
        assert ta.dtype == np.float32 and tb.dtype == np.float32
        return (ta.astype(np.float64).sum(1), np.abs(ta).astype(np.float64).sum(1),
                tb.astype(np.float64).sum(), np.abs(tb).astype(np.float64).sum())


def _mb_factor(mb, n_bits, sb):
    r = float(np.float32(mb).round())
    hi = n_bits - sb
    if not 1.0 <= r <= hi:
        return 0.0
    return math.log(2.0) * (-1.0 - (-math.log(2.0) * 2.0 ** (hi - r) + 2.0 ** -r / (2.0 - 2.0 ** -r)))


def _workspace_is_zero(x):
    from fp8q import ops
    ws = [w for k, w in ops._ws_cache.items() if k[0] == x.device.index and k[3] == "grad"]
    assert ws, "quantize_backward did not allocate its workspace"
    return all(int(w.count_nonzero()) == 0 for w in ws)


def _data(C, inner, per_channel, seed, specials=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(C, inner, generator=gen) * 0.8
    g = torch.randn(C, inner, generator=gen)
    mv = (torch.randn(C, generator=gen).abs() + 0.3) if per_channel else torch.tensor([1.3])
    if specials:
        flat, n = x.view(-1), x.numel()
        vals = [0.0, -0.0, 1e-40, -1e-42, 1e-30]
        for i, v in enumerate(vals):
            flat[(7 * i + 3) % n] = v
        m = mv.view(-1, 1) if per_channel else mv
        cols = torch.arange(C) % inner
        x[torch.arange(C), cols] = (m.expand(C, 1)[:, 0])                  # exactly on +maxval
        if inner > 1:
            x[torch.arange(C), (cols + 1) % inner] = -(m.expand(C, 1)[:, 0])   # exactly on -maxval (signed: a bound)
        g.view(-1)[5 % n] = 0.0
        g.view(-1)[11 % n] = 1e-41
    return x.cuda(), g.cuda(), mv.cuda()


def _check(x, g, mv, mb, n_bits, sb, per_channel, monkeypatch, what):
    from fp8q import ops
    y, cgx, cgmv, cgmb = _chain(x, g, mv, mb, n_bits, sb, monkeypatch)
    gx, gmv, gmb = ops.quantize_backward(x, g, mv, mb, n_bits, sb, True, True, True)
    assert _workspace_is_zero(x), what
    assert torch.equal(_bits(gx), _bits(cgx)), f"{what}: gx differs from the torch chain"
    sa, abs_a, sbm, abs_b = _host_sums(x, y, g, mv, sb, per_channel)
    got = gmv.cpu().numpy().astype(np.float64)
    fin = np.isfinite(sa)
    assert np.array_equal(np.isnan(got), np.isnan(sa)), what
    err = np.abs(got[fin] - sa[fin])
    assert (err <= BOUND * abs_a[fin]).all(), f"{what}: gmaxval off by {(err / np.maximum(abs_a[fin], 1e-300)).max():.3e} of sum|g w|"
    fac = _mb_factor(mb, n_bits, sb)
    got_b = float(gmb.cpu()[0])
    if fac == 0.0:
        assert got_b == 0.0, what
    elif np.isfinite(sbm):
        assert abs(got_b - fac * sbm) <= BOUND * abs(fac) * abs_b, f"{what}: gmbits {got_b} vs {fac * sbm}"
    else:
        assert not np.isfinite(got_b), what
    return gx, gmv, gmb


FORMATS = [(8, 2.0, 1), (8, 3.0, 1), (8, 3.0, 0), (6, 2.0, 1), (8, 5.0, 0)]


@pytest.mark.parametrize("n", [1, 3, 4097, (1 << 24) + 5])
def test_per_tensor_rows(n, monkeypatch):
    for k, (nb, mb, sb) in enumerate(FORMATS if n < (1 << 20) else FORMATS[:2]):
        x, g, mv = _data(1, n, False, 100 + k)
        _check(x.view(-1), g.view(-1), mv, mb, nb, sb, False, monkeypatch, f"per tensor n={n} fmt={nb, mb, sb}")


@pytest.mark.parametrize("C,inner", [(7, 9), (64, 147), (5, 4099), (1 << 16, 27), (3, 1), (130, 600)])
def test_per_channel_rows(C, inner, monkeypatch):
    for k, (nb, mb, sb) in enumerate(FORMATS):
        x, g, mv = _data(C, inner, True, 200 + k)
        _check(x, g, mv, mb, nb, sb, True, monkeypatch, f"per channel [{C},{inner}] fmt={nb, mb, sb}")
    x, g, mv = _data(C, inner, True, 210)                       # the same tensor with one range: a per-tensor call
    _check(x, g, mv[:1].clone(), 2.0, 8, 1, False, monkeypatch, f"per tensor [{C},{inner}]")


@pytest.mark.parametrize("per_channel", [False, True])
def test_nonfinite_inputs(per_channel, monkeypatch):
    C, inner = (6, 300) if per_channel else (1, 5000)
    x, g, mv = _data(C, inner, per_channel, 300)
    xf = x.view(-1)
    xf[17], xf[18], xf[19], xf[40] = float("nan"), float("inf"), float("-inf"), float("nan")
    g.view(-1)[17] = -2.0                                        # g * 0 keeps its sign
    if per_channel:
        xf[2 * inner + 5] = float("inf")                         # rows 2..: finite sums (an infinity clamps like any value)
    for nb, mb, sb in FORMATS[:3]:
        gx, gmv, _ = _check(x, g, mv, mb, nb, sb, per_channel, monkeypatch, f"non-finite pc={per_channel} fmt={nb, mb, sb}")
        assert float(gx.view(-1)[17]) == 0.0 and float(gx.view(-1)[40]) == 0.0
        assert bool(torch.isnan(gmv[0]))
        if per_channel:
            assert bool(torch.isfinite(gmv[1:]).all())


@pytest.mark.parametrize("C,inner,per_channel", [(1, 4097, False), (1, 70001, False), (64, 147, True), (5, 4099, True), (9, 27, True)])
def test_unaligned_pointers(C, inner, per_channel, monkeypatch):
    """x, g and gx each 4 bytes off a 16-byte boundary, in every combination of phases"""
    from fp8q import ops
    x0, g0, mv = _data(C, inner, per_channel, 400)
    n = x0.numel()
    shape = x0.shape if per_channel else (n,)
    ref = None
    for ox, og, oo in [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3), (3, 1, 2)]:
        bx, bg, bo = (torch.empty(n + 4, device="cuda") for _ in range(3))
        x, g, o = bx[ox:ox + n].view(shape), bg[og:og + n].view(shape), bo[oo:oo + n].view(shape)
        assert x.data_ptr() % 16 == 4 * ox and g.data_ptr() % 16 == 4 * og and o.data_ptr() % 16 == 4 * oo
        x.copy_(x0.view(shape))
        g.copy_(g0.view(shape))
        bo.fill_(float("nan"))
        gx, gmv, gmb = ops.quantize_backward(x, g, mv, 3.0, 8, 1, True, True, True, out=o)
        assert gx.data_ptr() == o.data_ptr()
        assert bool(torch.isnan(bo[:oo]).all()) and bool(torch.isnan(bo[oo + n:]).all()), "wrote outside gx"
        if ref is None:
            ref = _check(x, g, mv, 3.0, 8, 1, per_channel, monkeypatch, f"aligned [{C},{inner}]")
        for a, b in zip((gx, gmv, gmb), ref):
            assert torch.equal(_bits(a), _bits(b)), f"phases {ox, og, oo}: result depends on the alignment"
        assert _workspace_is_zero(x)


@pytest.mark.parametrize("C,inner,per_channel", [(1, 100003, False), (64, 147, True), (5, 4099, True), (300, 27, True)])
def test_output_subsets_widths_and_determinism(C, inner, per_channel, monkeypatch):
    from fp8q import ops
    x, g, mv = _data(C, inner, per_channel, 500)
    if not per_channel:
        x, g = x.view(-1), g.view(-1)
    full = _check(x, g, mv, 3.0, 8, 1, per_channel, monkeypatch, f"[{C},{inner}]")
    again = ops.quantize_backward(x, g, mv, 3.0, 8, 1, True, True, True)
    for a, b in zip(full, again):
        assert torch.equal(_bits(a), _bits(b)), "two calls on the same buffers differ"
    for need in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)]:
        res = ops.quantize_backward(x, g, mv, 3.0, 8, 1, *need)
        assert _workspace_is_zero(x)
        for want, a, b in zip(need, res, full):
            assert (a is not None) == want
            if want:
                assert torch.equal(_bits(a), _bits(b)), f"outputs {need}: differs from the call with all three"
    # host width against device width
    for mb in (3.0, 2.5, 0.2, 9.0, 1.0, 7.0):
        host = _check(x, g, mv, mb, 8, 1, per_channel, monkeypatch, f"[{C},{inner}] width {mb}")
        dev = ops.quantize_backward(x, g, mv, torch.tensor([mb], device="cuda"), 8, 1, True, True, True)
        assert _workspace_is_zero(x)
        for a, b in zip(host, dev):
            assert torch.equal(_bits(a), _bits(b)), f"width {mb}: host and device width differ"
        if mb in (0.2, 9.0):
            assert float(host[2][0]) == 0.0                      # the clamp cuts it off: exactly 0
    # unsigned, device width
    host = _check(x, g, mv, 4.0, 8, 0, per_channel, monkeypatch, f"[{C},{inner}] unsigned")
    dev = ops.quantize_backward(x, g, mv, torch.tensor([4.0], device="cuda"), 8, 0, True, True, True)
    for a, b in zip(host, dev):
        assert torch.equal(_bits(a), _bits(b))


def test_dense_non_contiguous_layout_per_tensor(monkeypatch):
    """channels-last x and g: the kernel runs on the storage as it lies, gx keeps the strides"""
    from fp8q import ops
    x, g, mv = _data(1, 8 * 16 * 6 * 6, False, 600)
    x = x.view(8, 16, 6, 6).contiguous(memory_format=torch.channels_last)
    g = g.view(8, 16, 6, 6).contiguous(memory_format=torch.channels_last)
    gx, gmv, gmb = ops.quantize_backward(x, g, mv, 3.0, 8, 1, True, True, True)
    assert gx.stride() == x.stride()
    y, cgx, cgmv, cgmb = _chain(x, g, mv, 3.0, 8, 1, monkeypatch)
    assert torch.equal(_bits(gx), _bits(cgx.contiguous(memory_format=torch.channels_last)))
    sa, abs_a, _, _ = _host_sums(x, y, g, mv, 1, False)
    assert abs(float(gmv[0]) - sa[0]) <= BOUND * abs_a[0]
