"""The INT backward kernel (fp8q_int_quantize_bwd_f32 through fp8q.ops.int_quantize_backward) against the torch op chain
    y = scale * (clamp(round_ste(x / scale) + zp, lo, hi) - zp),  scale = clamp(delta, min=eps),  zp = clamp(round_ste(zero_float), lo, hi)
written out below with plain torch ops and run by autograd on the same device buffers.

  gx                     bit-identical to g * m (m formed in numpy from the contract of include/fp8q.h); the same zero set as
                         the chain's gx, and |gx - chain| <= 2^-23 |chain| (the chain forms (g * scale) * m / scale: 1 ULP);
  gdelta, gzero_float    against a float64 host sum of the SAME fp32 per-element terms (formed in numpy in the contract's
                         order): |difference| <= 2^-22 * sum |term| per row -- exact fp32 terms, fp64 accumulation, one final
                         fp32 rounding (2^-24 relative) leave a factor of four to spare (the bound of test_grad_kernels.py);
                         with gradient scaling one more fp32 rounding: 2^-21.
                         The chain's own fp32 sums are cross-checked loosely (1e-5 of sum |g| (|v - zp| + |m t|), resp. of
                         sum |g scale|: the chain's 1-ULP terms and its fp32 summation): both mean the same quantity.

Every row that is long enough holds elements exactly on scale * (lo - zp) and scale * (hi - zp), a half-step tie, +-0, a
denormal, and upstream entries of 0 and 1e-41.  The 1e-41 sits on a CLIPPED element (m = 0): it goes through both sums as a
denormal product, while on an element with m = 1 the chain's own (g * scale) / scale would lose most of its bits in the
subnormal product and could not serve as a 1-ULP yardstick.  A second element, clipped at the other end under an ordinary
g, keeps every such row's gzero_float a normal number: the bounds are relative, and fp32 holds no denormal to 2^-21.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -22
BOUND_SCALED = 2.0 ** -21
F32 = np.float32
EPS = 1e-8

# (name, symmetric, signed, n_bits)
CONFIGS = [("asym8", False, False, 8), ("asym4", False, False, 4), ("sym_signed", True, True, 8), ("sym_unsigned", True, False, 8)]


class _RoundSTE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return torch.round(x)

    @staticmethod
    def backward(ctx, grad):
        return grad


def _grid(n_bits, symmetric, signed):
    if symmetric and signed:
        return F32(-2.0 ** (n_bits - 1)), F32(2.0 ** (n_bits - 1) - 1)
    return F32(0.0), F32(2.0 ** n_bits - 1)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _chain(x, g, delta, zf, n_bits, symmetric, signed):
    """(gx, gdelta, gzero_float) of autograd over the op chain, on x's device"""
    lo, hi = (float(v) for v in _grid(n_bits, symmetric, signed))
    xt, dt = x.clone().requires_grad_(True), delta.clone().requires_grad_(True)
    zt = None if symmetric else zf.clone().requires_grad_(True)
    shape = [-1] + [1] * (x.dim() - 1) if delta.numel() > 1 else [1]
    scale = torch.clamp(dt, min=EPS).view(shape)
    zp = 0.0 if symmetric else torch.clamp(_RoundSTE.apply(zt), lo, hi).view(shape)
    y = scale * (torch.clamp(_RoundSTE.apply(xt / scale) + zp, lo, hi) - zp)
    y.backward(g)
    return xt.grad, dt.grad, None if symmetric else zt.grad


def _host(x, g, delta, zf, n_bits, symmetric, signed):
    """The contract in numpy: g * m, and per row the float64 sums of the fp32 terms and of their magnitudes, masks applied"""
    C = delta.size
    lo, hi = _grid(n_bits, symmetric, signed)
    xr, gr = x.reshape(C, -1), g.reshape(C, -1)
    with np.errstate(all="ignore"):
        scale = np.maximum(delta, F32(EPS)).reshape(C, 1)
        zp = np.zeros((C, 1), F32) if symmetric else np.clip(np.rint(zf), lo, hi).reshape(C, 1)
        t = xr / scale
        u = np.rint(t) + zp
        m = ((u >= lo) & (u <= hi)).astype(F32)
        v = np.clip(u, lo, hi)
        w = (v - zp) - m * t
        ta, tb = gr * w, (F32(1.0) - m) * (gr * scale)
        gx = gr * m
        assert all(a.dtype == np.float32 for a in (t, u, v, w, ta, tb, gx))
        sa, abs_a = ta.astype(np.float64).sum(1), np.abs(ta).astype(np.float64).sum(1)
        sb, abs_b = tb.astype(np.float64).sum(1), np.abs(tb).astype(np.float64).sum(1)
        # what the chain's own roundings scale with: it adds g (v - zp) and -g' m t with g' = (g scale) / scale, 1 ULP off g
        loose_a = (np.abs(gr) * (np.abs(v - zp) + np.abs(m * t))).astype(np.float64).sum(1)
        loose_b = np.abs(gr * scale).astype(np.float64).sum(1)
    sa = np.where(delta >= F32(EPS), sa, 0.0)
    if not symmetric:
        rz = np.rint(zf)
        sb = np.where((rz >= lo) & (rz <= hi), -sb, 0.0)
    return gx.reshape(x.shape), sa, abs_a, sb, abs_b, loose_a, loose_b


def _data(C, inner, per_channel, cfg, seed, specials=True):
    """numpy x, g [C, inner] and the ranges (about 0.7 x the data's min / max, so both ends clip)"""
    _, symmetric, signed, n_bits = cfg
    rng = np.random.RandomState(seed)
    x = (rng.randn(C, inner) * 0.8).astype(F32)
    g = rng.randn(C, inner).astype(F32)
    rows = x if per_channel else x.reshape(1, -1)
    mn, mx = np.minimum(rows.min(1), F32(-0.05)), np.maximum(rows.max(1), F32(0.05))
    lo, hi = _grid(n_bits, symmetric, signed)
    if symmetric:
        delta = (F32(0.7) * (np.maximum(-mn, mx) if signed else mx) / hi).astype(F32)
        zf = None
    else:
        delta = (F32(0.7) * (mx - mn) / hi).astype(F32)
        zf = (F32(-0.7) * mn / delta).astype(F32)
    if specials:
        R = rows.shape[0]
        L = rows.shape[1]
        scale = np.maximum(delta, F32(EPS))
        zp = np.zeros(R, F32) if symmetric else np.clip(np.rint(zf), lo, hi)
        vals = [scale * (lo - zp), scale * (hi - zp), F32(1.5) * scale, np.full(R, 0.0, F32), np.full(R, -0.0, F32),
                np.full(R, 1e-40, F32)]
        grow = g if per_channel else g.reshape(1, -1)
        for i, v in enumerate(vals):
            if i < L:
                rows[:, i] = v.astype(F32)
        if L >= 8:
            grow[:, 6] = 0.0
            rows[:, 7] = F32(2.0) * mx + F32(1.0)          # clipped at the upper end: m = 0
            grow[:, 7] = F32(1e-41)
        if L >= 9:
            # clipped at the lower end under an ordinary g: every row's gzero_float sum is then a normal number, the
            # denormal product above one term of it.  Alone, that product times gs is a denormal whose fp32 spacing
            # (2^-149) no relative bound can hold.
            rows[:, 8] = F32(2.0) * mn - F32(1.0)
            grow[:, 8] = np.where(np.abs(grow[:, 8]) < F32(0.25), F32(0.25), grow[:, 8])
    return x, g, delta, zf


def _workspace_is_zero(x):
    from fp8q import ops
    ws = [w for k, w in ops._ws_cache.items() if k[0] == x.device.index and k[3] == "grad"]
    assert ws, "int_quantize_backward did not allocate its workspace"
    return all(int(w.count_nonzero()) == 0 for w in ws)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(x, g, delta, zf, cfg, what, gs_elems=0):
    """x, g, delta, zf: numpy.  Runs the kernel and the chain on the same device buffers; returns the kernel's results."""
    from fp8q import ops
    _, symmetric, signed, n_bits = cfg
    xd, gd_, dd, zd = _dev(x), _dev(g), _dev(delta), _dev(zf)
    flag = torch.tensor([signed], dtype=torch.bool, device="cuda") if symmetric else None
    gx, gdl, gz = ops.int_quantize_backward(xd, gd_, dd, zd, flag, n_bits, symmetric, EPS, True, True, not symmetric, gs_elems)
    assert _workspace_is_zero(xd), what
    cgx, cgd, cgz = _chain(xd, gd_, dd, zd, n_bits, symmetric, signed)
    hgx, sa, abs_a, sb, abs_b, loose_a, loose_b = _host(x, g, delta, zf, n_bits, symmetric, signed)
    # gx
    assert torch.equal(_bits(gx), _bits(_dev(hgx))), f"{what}: gx is not g * m to the bit"
    got, ref = gx.cpu().numpy().astype(np.float64), cgx.cpu().numpy().astype(np.float64)
    assert np.array_equal(got == 0, ref == 0), f"{what}: gx and the chain's gx vanish on different elements"
    assert (np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref)).all(), f"{what}: gx off the chain by {np.abs(got - ref).max():.3e}"
    # the sums
    lo, hi = _grid(n_bits, symmetric, signed)
    gs = float(F32(1.0 / np.sqrt(float(hi) * gs_elems))) if gs_elems else 1.0
    bound = BOUND_SCALED if gs_elems else BOUND
    for name, k, c, s, mag, loose in (("gdelta", gdl, cgd, sa, abs_a, loose_a), ("gzero_float", gz, cgz, sb, abs_b, loose_b)):
        if k is None:
            assert symmetric and name == "gzero_float"
            continue
        got = k.cpu().numpy().astype(np.float64).reshape(-1)
        fin = np.isfinite(s)
        assert np.array_equal(np.isnan(got), np.isnan(s)), f"{what}: {name} NaN rows differ"
        err = np.abs(got[fin] - gs * s[fin])
        print(f"{what}: {name} worst {float((err / np.maximum(gs * mag[fin], 1e-300)).max()) if err.size else 0.0:.3e} of sum |term| (bound {bound:.2e})")
        assert (err <= bound * gs * mag[fin]).all(), f"{what}: {name} off by {(err / np.maximum(gs * mag[fin], 1e-300)).max():.3e} of sum |term|"
        assert (got[s == 0] == 0).all(), f"{what}: {name} is not exactly 0 where the contract says so"
        ch = c.cpu().numpy().astype(np.float64).reshape(-1)
        assert np.array_equal(np.isnan(ch), np.isnan(s)), f"{what}: the chain's {name} has other NaN rows"
        assert (np.abs(ch[fin] - s[fin]) <= 1e-5 * loose[fin] + 1e-30).all(), f"{what}: the chain's {name} means something else"
    return gx, gdl, gz


@functools.lru_cache(maxsize=None)
def _case(C, inner, per_channel, ci):
    return _data(C, inner, per_channel, CONFIGS[ci], 1000 + 17 * ci + C % 97 + inner % 89)


@pytest.mark.parametrize("ci", range(len(CONFIGS)), ids=[c[0] for c in CONFIGS])
@pytest.mark.parametrize("n", [1, 3, 4097, 3 * 4096 + 5])
def test_per_tensor_rows(n, ci):
    x, g, delta, zf = _case(1, n, False, ci)
    _check(x.reshape(-1), g.reshape(-1), delta, zf, CONFIGS[ci], f"per tensor n={n} {CONFIGS[ci][0]}")
    _check(x.reshape(-1), g.reshape(-1), delta, zf, CONFIGS[ci], f"per tensor n={n} {CONFIGS[ci][0]} scaled", gs_elems=n)


@pytest.mark.parametrize("ci", range(len(CONFIGS)), ids=[c[0] for c in CONFIGS])
@pytest.mark.parametrize("C,inner", [(3, 1), (7, 9), (64, 147), (5, 4099), (130, 600), (70000, 5)])
def test_per_channel_rows(C, inner, ci):
    x, g, delta, zf = _case(C, inner, True, ci)
    _check(x, g, delta, zf, CONFIGS[ci], f"per channel [{C},{inner}] {CONFIGS[ci][0]}")
    _check(x, g, delta, zf, CONFIGS[ci], f"per channel [{C},{inner}] {CONFIGS[ci][0]} scaled", gs_elems=inner)
    if ci == 0:                                                   # the same tensor with one range: a per-tensor call
        d1, z1 = delta[:1].copy(), zf[:1].copy()
        _check(x, g, d1, z1, CONFIGS[ci], f"per tensor [{C},{inner}]")


@pytest.mark.parametrize("ci", range(len(CONFIGS)), ids=[c[0] for c in CONFIGS])
@pytest.mark.parametrize("C,inner", [(6, 300), (4, 5000)])
def test_nonfinite_rows(C, inner, ci):
    """a NaN in row 0, +inf in row 1: those rows' gdelta is NaN, gx is 0 there, the other rows are unaffected"""
    x, g, delta, zf = (None if a is None else a.copy() for a in _case(C, inner, True, ci))
    clean = _check(x, g, delta, zf, CONFIGS[ci], f"finite [{C},{inner}] {CONFIGS[ci][0]}")
    x[0, 17], x[1, 40] = np.nan, np.inf
    g[0, 17] = -2.0
    gx, gdl, gz = _check(x, g, delta, zf, CONFIGS[ci], f"non-finite [{C},{inner}] {CONFIGS[ci][0]}")
    assert float(gx[0, 17]) == 0.0 and float(gx[1, 40]) == 0.0
    assert bool(torch.isnan(gdl[:2]).all()) and bool(torch.isfinite(gdl[2:]).all())
    assert torch.equal(_bits(gdl[2:]), _bits(clean[1][2:]))
    if gz is not None:
        assert bool(torch.isfinite(gz).all()) and torch.equal(_bits(gz[2:]), _bits(clean[2][2:]))


@pytest.mark.parametrize("C,inner", [(7, 9), (130, 600), (5, 4099)])
def test_masked_channels(C, inner):
    """delta below eps: gdelta exactly 0; rint(zero_float) outside [lo, hi]: gzero_float exactly 0"""
    for ci in (0, 1, 2):
        x, g, delta, zf = (None if a is None else a.copy() for a in _case(C, inner, True, ci))
        delta[1] = 1e-9
        if zf is not None:
            zf[2], zf[3] = float(_grid(CONFIGS[ci][3], False, False)[1]) + 5.0, -3.0
        _, gdl, gz = _check(x, g, delta, zf, CONFIGS[ci], f"masked [{C},{inner}] {CONFIGS[ci][0]}")
        assert float(gdl[1]) == 0.0 and float(gdl[0]) != 0.0
        if gz is not None:
            assert float(gz[2]) == 0.0 and float(gz[3]) == 0.0 and float(gz[4]) != 0.0
        _, gdl, gz = _check(x, g, delta, zf, CONFIGS[ci], f"masked scaled [{C},{inner}] {CONFIGS[ci][0]}", gs_elems=inner)
        assert float(gdl[1]) == 0.0


@pytest.mark.parametrize("C,inner,per_channel", [(1, 4097, False), (1, 3 * 4096 + 5, False), (64, 147, True), (5, 4099, True), (7, 9, True)])
def test_views_at_odd_offsets_subsets_and_determinism(C, inner, per_channel):
    """x, g and gx each 4 bytes off a 16-byte boundary in several combinations; every subset of the outputs; two calls"""
    from fp8q import ops
    for ci in (0, 2):
        cfg = CONFIGS[ci]
        _, symmetric, signed, n_bits = cfg
        x0, g0, delta, zf = _case(C, inner, per_channel, ci)
        shape = (C, inner) if per_channel else (C * inner,)
        ref = _check(x0.reshape(shape), g0.reshape(shape), delta, zf, cfg, f"aligned {shape} {cfg[0]}")
        n = C * inner
        dd, zd = _dev(delta), _dev(zf)
        flag = torch.tensor([signed], dtype=torch.bool, device="cuda") if symmetric else None
        call = lambda x, g, *need, **kw: ops.int_quantize_backward(x, g, dd, zd, flag, n_bits, symmetric, EPS, *need, **kw)
        for ox, og, oo in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3), (3, 1, 2)]:
            bx, bg, bo = (torch.empty(n + 4, device="cuda") for _ in range(3))
            x, g, o = bx[ox:ox + n].view(shape), bg[og:og + n].view(shape), bo[oo:oo + n].view(shape)
            assert x.data_ptr() % 16 == 4 * ox and g.data_ptr() % 16 == 4 * og and o.data_ptr() % 16 == 4 * oo
            x.copy_(_dev(x0).view(shape))
            g.copy_(_dev(g0).view(shape))
            bo.fill_(float("nan"))
            res = call(x, g, True, True, not symmetric, out=o)
            assert res[0].data_ptr() == o.data_ptr()
            assert bool(torch.isnan(bo[:oo]).all()) and bool(torch.isnan(bo[oo + n:]).all()), "wrote outside gx"
            for a, b in zip(res, ref):
                assert (a is None) == (b is None)
                if a is not None:
                    assert torch.equal(_bits(a), _bits(b)), f"phases {ox, og, oo}: the result depends on the alignment"
            assert _workspace_is_zero(x)
        x, g = _dev(x0).view(shape), _dev(g0).view(shape)
        again = call(x, g, True, True, not symmetric)
        for a, b in zip(again, ref):
            assert (a is None) == (b is None) and (a is None or torch.equal(_bits(a), _bits(b))), "two calls differ"
        needs = [(True, False, False), (False, True, False), (True, True, False)]
        if not symmetric:
            needs += [(False, False, True), (False, True, True), (True, False, True)]
        for need in needs:
            res = call(x, g, *need)
            assert _workspace_is_zero(x)
            for want, a, b in zip(need, res, ref):
                assert (a is not None) == want
                if want:
                    assert torch.equal(_bits(a), _bits(b)), f"outputs {need}: differs from the call with all of them"


def test_dense_non_contiguous_layout_per_tensor():
    """channels-last x and g: the kernel runs on the storage as it lies, gx keeps the strides"""
    from fp8q import ops
    x0, g0, delta, zf = _case(1, 8 * 16 * 6 * 6, False, 0)
    x = _dev(x0).view(8, 16, 6, 6).contiguous(memory_format=torch.channels_last)
    g = _dev(g0).view(8, 16, 6, 6).contiguous(memory_format=torch.channels_last)
    dd, zd = _dev(delta), _dev(zf)
    gx, gdl, gz = ops.int_quantize_backward(x, g, dd, zd, None, 8, False, EPS, True, True, True)
    assert gx.stride() == x.stride()
    hgx, sa, abs_a, sb, abs_b, _, _ = _host(x.contiguous().cpu().numpy(), g.contiguous().cpu().numpy(), delta, zf, 8, False, False)
    assert torch.equal(_bits(gx.contiguous()), _bits(_dev(hgx)))
    assert abs(float(gdl[0]) - sa[0]) <= BOUND * abs_a[0] and abs(float(gz[0]) - sb[0]) <= BOUND * abs_b[0]
