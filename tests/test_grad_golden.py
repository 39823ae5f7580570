"""The FP quantizer's gradient against the reference's own CPU autograd: g10_autograd.npz through the kernel route, and the
new fixture g14_grad.npz (tests/golden/make_golden_grad.py) through the torch chain on the CPU oracle backend and through the
kernel route on the GPU, with the same bounds.

Bounds of the g14 comparison, the same for all 120 cases (5 layouts x 24 formats, none left out) and for both routes:
  gx        same zero set, |got - ref| <= 2.5e-7 |ref| + a_i: the reference's chain forms the 0 / 0.5 / 1 mask as (g * s) / s,
            1 ULP of noise (as g10).  a_i is the reference's own error where its g_i * s is SUBNORMAL, and 0 everywhere else:
            the smallest scale of a row is s_min = 2^(1 - M - bias), bias = 2^E - log2(maxval) + log2(2 - 2^-M) - 1; a
            product with |g_i| s_min >= 2^-126 is normal whatever the element's scale (a_i = 0); otherwise it is rounded to
            the subnormal spacing 2^-149, an error <= 2^-150, which the division by s >= s_min turns into
            a_i = 1.01 * 2^-150 / s_min (1 % for the reference's fp32 s).  Only E = 7 (n_bits 8, unsigned, width 1:
            s_min ~ 2^-127 ... 2^-129) has such elements; there a_i ~ 1e-7 ... 6e-7.
  gmaxval   per row  |got - ref| <= K_SUM * sum_i |g_i| |w_i| + T     (w_i evaluated in float64 from the route's own forward)
  gmbits             |got - ref| <= K_SUM * |factor| * sum_i |g_i| |y_i - xc_i| + |factor| * maxval * T
            an absolute bound relative to the sum of magnitudes: the terms have both signs and cancel.  K_SUM is four times the
            largest ratio the oracle-backed torch chain shows against the fixture on the CPU (test_g14_torch_chain_on_oracle_cpu
            prints it): the factor covers the <= 2-ULP forward difference between oracle and reference on ~1.8 % of the
            elements -- a difference of the size of the term itself wherever y - xc is a rounding residue -- and another
            summation order.
            T is the tie term of E = 0 (n_bits 6, signed, width 5) and 0 for every other format: with E = 0 the one scale is
            s = maxval / (2^M - 1/2), so every element with |x| >= maxval has xc / s EXACTLY on the rounding tie 2^M - 1/2,
            and the last bit of s -- the reference's `pow` -- decides whether y is 2^M s or (2^M - 1) s (DESIGN.md section
            2).  Two correct forwards therefore differ by one grid step s on such an element, its term g (y - xc) / maxval
            by |g| s / maxval:  T = sum over the row's elements with |x| >= maxval of |g_i| / (2^M - 1/2)
            (for gmbits the same sum over all rows, each row's with its own maxval).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

MEASURED_RATIO = 4.77e-6     # largest |chain - reference| / sum of magnitudes over the 120 cases, CPU: gmbits of [96,1,3,3] E2M5 (gmaxval rows: 3.69e-6)
K_SUM = 4 * MEASURED_RATIO


def _load(golden_dir):
    g = np.load(os.path.join(golden_dir, "g14_grad.npz"))
    return g, json.loads(str(g["cases"]))


def _mask_times_g(x, g, mv, sb):
    lo = -mv if sb == 1 else np.zeros_like(mv)
    m = ((x > lo) & (x < mv)).astype(np.float32) + np.float32(0.5) * ((x == mv) | (x == lo)).astype(np.float32)
    return (g * m).astype(np.float32)


def _case(g, c):
    x, up, mv = g[f"x_{c['shape']}"], g[f"g_{c['shape']}"], g[f"maxval_{c['layout']}"]
    mvb = mv.reshape([-1] + [1] * (x.ndim - 1)) if c["per_channel"] else mv
    gx = (g[f"gxx_{c['gx']}"] ^ _mask_times_g(x, up, mvb, c["sign_bits"]).view(np.uint32)).view(np.float32)
    return x, up, mv, gx, g[f"c{c['k']}_gmaxval"], g[f"c{c['k']}_gmbits"]


def _magnitudes(x, y, up, mv, c):
    """float64: per row sum |g| |w| and the tie term T; |factor| * sum |g| |y - xc| and its tie term"""
    C = mv.size if c["per_channel"] else 1
    x, y, up = (a.astype(np.float64).reshape(C, -1) for a in (x, y, up))
    m = mv.astype(np.float64).reshape(C, 1)
    sb = c["sign_bits"]
    lo = -m if sb == 1 else np.zeros_like(m)
    d = y - np.minimum(np.maximum(x, lo), m)
    w = d / m + (x > m) + 0.5 * (x == m)
    if sb == 1:
        w = w - (x < lo) - 0.5 * (x == lo)
    r, hi = float(np.float32(c["mbits"]).round()), c["n_bits"] - sb
    fac = math.log(2.0) * (-1.0 - (-math.log(2.0) * 2.0 ** (hi - r) + 2.0 ** -r / (2.0 - 2.0 ** -r)))
    tie = np.zeros(C)
    if hi - r == 0:
        tie = (np.abs(up) * (np.abs(x) >= m)).sum(1) / (2.0 ** r - 0.5)
    return (np.abs(up) * np.abs(w)).sum(1), tie, abs(fac) * (np.abs(up) * np.abs(d)).sum(), abs(fac) * (tie * m[:, 0]).sum()


def _gx_atol(up, mv, c):
    """a_i of the module docstring, shaped like up"""
    C = mv.size if c["per_channel"] else 1
    M = float(np.float32(c["mbits"]).round())
    E = c["n_bits"] - c["sign_bits"] - M
    bias = 2.0 ** E - np.log2(mv.astype(np.float64)) + math.log2(2.0 - 2.0 ** -M) - 1.0
    s_min = (2.0 ** (1.0 - M - bias)).reshape(C, 1)
    g = np.abs(up.astype(np.float64)).reshape(C, -1)
    return np.where(g * s_min < 2.0 ** -126, 1.01 * 2.0 ** -150 / s_min, 0.0).reshape(up.shape)


def _run(x, up, mv, c, dev):
    from quantization.quantizers.fp8_quantizer import quantize_to_fp8_ste_MM
    xt = torch.from_numpy(x.copy()).to(dev).requires_grad_(True)
    mt = torch.from_numpy(mv.copy()).to(dev).requires_grad_(True)
    bt = torch.Tensor([c["mbits"]]).requires_grad_(True)
    y = quantize_to_fp8_ste_MM(xt, c["n_bits"], mt, bt, c["sign_bits"])
    y.backward(torch.from_numpy(up).to(dev))
    return y.detach().cpu().numpy(), xt.grad.cpu().numpy(), mt.grad.cpu().numpy(), bt.grad.cpu().numpy()


def _check_g14(golden_dir, dev):
    g, cases = _load(golden_dir)
    assert len(cases) == 120
    worst = 0.0
    for c in cases:
        x, up, mv, gx_ref, gmv_ref, gmb_ref = _case(g, c)
        what = f"case {c}"
        y, gx, gmv, gmb = _run(x, up, mv, c, dev)
        np.testing.assert_array_equal(gx == 0, gx_ref == 0, err_msg=what)
        err = np.abs(gx.astype(np.float64) - gx_ref)
        a = _gx_atol(up, mv, c)
        over = err > 2.5e-7 * np.abs(gx_ref.astype(np.float64)) + a
        print(f"{c['layout']} n_bits={c['n_bits']} mbits={c['mbits']} sign={c['sign_bits']}: gx max abs error {err.max():.3e}, "
              f"{int((a > 0).sum())} elements with a subnormal g * s (a_i up to {a.max():.2e})")
        assert not over.any(), f"{what}: gx off by {err[over].max():.3e} on {int(over.sum())} elements"
        mag_a, tie_a, mag_b, tie_b = _magnitudes(x, y, up, mv, c)
        da = np.abs(gmv.astype(np.float64).reshape(-1) - gmv_ref.reshape(-1))
        db = abs(float(gmb[0]) - float(gmb_ref[0]))
        ra = np.maximum(da - tie_a, 0.0) / mag_a
        rb = max(db - tie_b, 0.0) / mag_b
        worst = max(worst, float(ra.max()), rb)
        print(f"    gmaxval {ra.max():.3e}  gmbits {rb:.3e} of the sums of magnitudes"
              + (f"   (E = 0: |diff| up to {da.max():.3e} / {db:.3e}, tie terms up to {tie_a.max():.3e} / {tie_b:.3e})" if tie_b else ""))
        assert (ra <= K_SUM).all(), f"{what}: gmaxval off by {ra.max():.3e} of sum |g||w| (bound {K_SUM:.1e})"
        assert rb <= K_SUM, f"{what}: gmbits off by {rb:.3e} of |factor| sum |g||y - xc| (bound {K_SUM:.1e})"
    print(f"largest ratio on {dev}: {worst:.3e} (K_SUM = {K_SUM:.1e})")
    return worst


def test_g14_fixture_shape(golden_dir):
    g, cases = _load(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "g14_grad.npz")) < 1_000_000
    layouts = {(c["layout"], c["per_channel"]) for c in cases}
    assert layouts == {("w7_pc", 1), ("w7_pt", 0), ("dw_pc", 1), ("act_pt", 0), ("odd_pc", 1)}
    assert g["x_w7"].shape == (64, 3, 7, 7) and g["x_dw"].shape == (96, 1, 3, 3)
    assert g["x_act"].shape == (8, 32, 14, 14) and g["x_odd"].shape == (5, 1031)
    formats = {(nb, mb, sb) for nb in (8, 6) for mb in (1.0, 2.0, 3.0, 4.0, 5.0, 2.5) for sb in (1, 0)}
    for lid in ("w7_pc", "w7_pt", "dw_pc", "act_pt", "odd_pc"):       # every format on every layout, E = 0 and E = 7 too
        assert {(c["n_bits"], c["mbits"], c["sign_bits"]) for c in cases if c["layout"] == lid} == formats, lid
    assert len(cases) == 5 * 24
    for c in cases:                                   # every case has elements exactly on +-maxval and at 0
        x, mv = g[f"x_{c['shape']}"], g[f"maxval_{c['layout']}"]
        rows = x.reshape(mv.size if c["per_channel"] else 1, -1)
        m = mv.reshape(-1, 1)
        assert ((rows == m).any(1) & (rows == -m).any(1) & (rows == 0).any(1)).all(), c


def test_g14_torch_chain_on_oracle_cpu(golden_dir):
    """pins the tolerances: today's torch chain with the CPU oracle as the forward"""
    import oracle_ops
    with oracle_ops.patched():
        worst = _check_g14(golden_dir, "cpu")
    assert worst <= MEASURED_RATIO * 1.0001, f"MEASURED_RATIO is out of date: {worst:.3e}"


def _spy(monkeypatch):
    from fp8q import ops
    calls, real = [], ops.quantize_backward

    def spy(*a, **k):
        calls.append(a)
        return real(*a, **k)
    monkeypatch.setattr(ops, "quantize_backward", spy)
    return calls


@pytest.mark.gpu
def test_g14_kernel_route(golden_dir, monkeypatch):
    calls = _spy(monkeypatch)
    _check_g14(golden_dir, "cuda")
    assert len(calls) == 120, "the kernel route was not taken"


@pytest.mark.gpu
def test_g10_kernel_route(golden_dir, monkeypatch):
    """g10_autograd.npz with the tolerances of tests/test_autograd.py, and the proof that the kernel computed it"""
    import test_autograd
    calls = _spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, "g10_autograd.npz"))
    test_autograd._check(g, "cuda")
    assert len(calls) == len(g["cases"]) + len(g["mb_cases"])
    for a in calls:
        assert a[0].is_cuda and a[0].dtype == torch.float32


@pytest.mark.gpu
def test_g10_env_switch_keeps_the_torch_chain(golden_dir, monkeypatch):
    import test_autograd
    monkeypatch.setenv("FP8Q_GRAD_KERNELS", "0")
    calls = _spy(monkeypatch)
    test_autograd._check(np.load(os.path.join(golden_dir, "g10_autograd.npz")), "cuda")
    assert not calls
