"""The INT quantizers' gradient against the reference's own CPU autograd: gi1_int_grad.npz (tests/golden/make_golden_int_grad.py)
through the quantizers of quantization/uniform.py on the GPU -- the kernel route, and the torch chain under FP8Q_GRAD_KERNELS=0 --
with the same bounds for all 60 cases (5 layouts x {asymmetric, symmetric signed, symmetric one-sided} x n_bits {8, 4} x
grad_scaling {off, on}, none left out):

  gx                     the fixture's zero set, |got - ref| <= 2.5e-7 |ref| (the reference forms (g * scale) * m / scale: 1 ULP);
  gdelta, gzero_float    per row |got - ref| <= K_SUM * sum |term| (times gs with gradient scaling), the terms those of
                         include/fp8q.h evaluated in numpy.  K_SUM = 4 x MEASURED_RATIO, the largest distance of the float64
                         sum of the contract's fp32 terms from the fixture, measured on the CPU when the fixture was made
                         (test_gi1_measured_ratio_is_current keeps it current); the factor 4 is the margin for another
                         summation order.  The ratio is set by the rows of 9 elements of [96,1,3,3]: the reference adds
                         g (v - zp) and -g' t with g' = (g * scale) / scale one ULP off g, an error of |g| |t| 2^-24 -- |t| up
                         to 2^n_bits -- that a short row does not average out, next to terms |g| |v - zp - t| <= |g| / 2.
"""
import json
import os

import numpy as np
import pytest
import torch

MEASURED_RATIO = 1.718e-4    # largest |float64 sum of the contract's fp32 terms - reference| / sum |term| over the 60 cases, CPU: gdelta of [96,1,3,3] symmetric signed 8 bit
K_SUM = 4 * MEASURED_RATIO
F32 = np.float32
EPS = 1e-8


def _load(golden_dir):
    g = np.load(os.path.join(golden_dir, "gi1_int_grad.npz"))
    return g, json.loads(str(g["cases"]))


def _grid(c):
    if c["kind"] != "asym" and c["signed"]:
        return F32(-2.0 ** (c["n_bits"] - 1)), F32(2.0 ** (c["n_bits"] - 1) - 1)
    return F32(0.0), F32(2.0 ** c["n_bits"] - 1)


def _contract(x, g, delta, zf, c):
    """include/fp8q.h in numpy: g * m; per row the float64 sums of the fp32 terms (masks applied) and of their magnitudes"""
    C = delta.size
    lo, hi = _grid(c)
    xr, gr = x.reshape(C, -1), g.reshape(C, -1)
    scale = np.maximum(delta, F32(EPS)).reshape(C, 1)
    zp = np.zeros((C, 1), F32) if zf is None else np.clip(np.rint(zf), lo, hi).reshape(C, 1)
    t = xr / scale
    u = np.rint(t) + zp
    m = ((u >= lo) & (u <= hi)).astype(F32)
    w = (np.clip(u, lo, hi) - zp) - m * t
    ta, tb = gr * w, (F32(1) - m) * (gr * scale)
    assert ta.dtype == np.float32 and tb.dtype == np.float32
    sa, abs_a = ta.astype(np.float64).sum(1), np.abs(ta).astype(np.float64).sum(1)
    sb, abs_b = -tb.astype(np.float64).sum(1), np.abs(tb).astype(np.float64).sum(1)
    sa = np.where(delta >= F32(EPS), sa, 0.0)
    if zf is not None:
        rz = np.rint(zf)
        sb = np.where((rz >= lo) & (rz <= hi), sb, 0.0)
    return (gr * m).reshape(x.shape), sa, abs_a, sb, abs_b


def _case(g, c):
    """x (the shape's data with the case's leading row elements written in), upstream g, the ranges, the reference's results"""
    x = g[f"x_{c['shape']}"].copy()
    C = x.shape[0] if c["per_channel"] else 1
    x.reshape(C, -1)[:, :5] = g[c["x"]]
    up, k = g[f"g_{c['shape']}"], c["k"]
    delta = g[f"c{k}_delta"]
    asym = c["kind"] == "asym"
    zf = g[f"c{k}_zf"] if asym else None
    base = _contract(x, up, delta, zf, c)
    gx = (g[f"gxx_{c['gx']}"] ^ base[0].view(np.uint32)).view(np.float32)
    n_el = x.size // x.shape[0] if c["per_channel"] else x.size
    gs = float(F32(1.0 / np.sqrt(float(_grid(c)[1]) * n_el))) if c["grad_scaling"] else 1.0
    return x, up, delta, zf, gx, g[f"c{k}_gdelta"], (g[f"c{k}_gzf"] if asym else None), base, gs


def _ratio(diff, mag):
    """largest |diff| / mag over the rows; a row without terms must agree exactly"""
    diff = np.abs(np.asarray(diff, np.float64))
    assert (diff[mag == 0] == 0).all()
    return float((diff[mag > 0] / mag[mag > 0]).max()) if (mag > 0).any() else 0.0


def test_gi1_fixture_shape(golden_dir):
    g, cases = _load(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "gi1_int_grad.npz")) < 1_000_000
    assert g["x_w7"].shape == (64, 3, 7, 7) and g["x_dw"].shape == (96, 1, 3, 3)
    assert g["x_act"].shape == (8, 32, 14, 14) and g["x_odd"].shape == (5, 1031)
    configs = {(k, nb, gs) for k in ("asym", "sym_signed", "sym_onesided") for nb in (8, 4) for gs in (0, 1)}
    for lid, pc in (("w7_pc", 1), ("w7_pt", 0), ("dw_pc", 1), ("act_pt", 0), ("odd_pc", 1)):
        mine = [c for c in cases if c["layout"] == lid]
        assert {(c["kind"], c["n_bits"], c["grad_scaling"]) for c in mine} == configs and len(mine) == 12, lid
        assert all(c["per_channel"] == pc for c in mine)
    assert len(cases) == 60
    for sid in ("w7", "dw", "act", "odd"):
        up = np.abs(g[f"g_{sid}"])
        assert (up == 0).any() and up[up > 0].min() >= 1e-20          # the reference's g * scale stays normal
    for c in cases:
        assert c["signed"] == (c["kind"] == "sym_signed")
        x, up, delta, zf, gx, gd, gz, base, gs = _case(g, c)
        assert np.array_equal(gx == 0, base[0] == 0), c                # the reference's mask is the contract's
        assert (gx == 0).any() and (gx != 0).any()
        assert (base[4] > 0).any(), c                                   # clipped elements


def test_gi1_measured_ratio_is_current(golden_dir):
    """pins the tolerance: the contract's terms, summed in float64 on the CPU, against the reference's results"""
    g, cases = _load(golden_dir)
    worst = 0.0
    for c in cases:
        x, up, delta, zf, gx, gd, gz, (_, sa, abs_a, sb, abs_b), gs = _case(g, c)
        ra = _ratio(gs * sa - gd, gs * abs_a)
        rb = _ratio(gs * sb - gz, gs * abs_b) if gz is not None else 0.0
        print(f"{c['layout']} {c['kind']} b{c['n_bits']} gs{c['grad_scaling']}: gdelta {ra:.3e}  gzero_float {rb:.3e} of the sums of magnitudes")
        worst = max(worst, ra, rb)
    print(f"largest ratio: {worst:.3e} (MEASURED_RATIO = {MEASURED_RATIO:.3e})")
    assert worst <= MEASURED_RATIO * 1.0001, f"MEASURED_RATIO is out of date: {worst:.3e}"
    assert worst >= MEASURED_RATIO * 0.99, f"MEASURED_RATIO is not the measured one: {worst:.3e}"


def _spy(monkeypatch):
    from fp8q import ops
    calls, real = [], ops.int_quantize_backward

    def spy(*a, **k):
        calls.append(a)
        return real(*a, **k)
    monkeypatch.setattr(ops, "int_quantize_backward", spy)
    return calls


def _check_gi1(golden_dir):
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    g, cases = _load(golden_dir)
    assert len(cases) == 60
    worst = 0.0
    for c in cases:
        x, up, delta, zf, gx_ref, gd_ref, gz_ref, (_, _, abs_a, _, abs_b), gs = _case(g, c)
        what = f"case {c}"
        asym = c["kind"] == "asym"
        q = (AsymmetricUniformQuantizer if asym else SymmetricUniformQuantizer)(
            n_bits=c["n_bits"], per_channel=bool(c["per_channel"]), grad_scaling=bool(c["grad_scaling"]))
        q._delta = torch.from_numpy(delta.copy()).cuda()
        if asym:
            q._zero_float = torch.from_numpy(zf.copy()).cuda()
        else:
            q._signed = torch.tensor(bool(c["signed"]), device="cuda")
        q.make_range_trainable()
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        q(xt).backward(torch.from_numpy(up).cuda())
        assert q._delta.grad.shape == q._delta.shape
        gx = xt.grad.cpu().numpy()
        np.testing.assert_array_equal(gx == 0, gx_ref == 0, err_msg=what)
        err = np.abs(gx.astype(np.float64) - gx_ref)
        assert (err <= 2.5e-7 * np.abs(gx_ref.astype(np.float64))).all(), f"{what}: gx off by {err.max():.3e}"
        ra = _ratio(q._delta.grad.cpu().numpy().reshape(-1) - gd_ref, gs * abs_a)
        rb = _ratio(q._zero_float.grad.cpu().numpy().reshape(-1) - gz_ref, gs * abs_b) if asym else 0.0
        print(f"{c['layout']} {c['kind']} b{c['n_bits']} gs{c['grad_scaling']}: gdelta {ra:.3e}  gzero_float {rb:.3e} of the sums of magnitudes")
        worst = max(worst, ra, rb)
        assert ra <= K_SUM, f"{what}: gdelta off by {ra:.3e} of sum |term| (bound {K_SUM:.1e})"
        assert rb <= K_SUM, f"{what}: gzero_float off by {rb:.3e} of sum |term| (bound {K_SUM:.1e})"
    print(f"largest ratio: {worst:.3e} (K_SUM = {K_SUM:.1e})")


@pytest.mark.gpu
def test_gi1_kernel_route(golden_dir, monkeypatch):
    calls = _spy(monkeypatch)
    _check_gi1(golden_dir)
    assert len(calls) == 60, "the kernel route was not taken once per case"
    for a in calls:
        assert a[0].is_cuda and a[0].dtype == torch.float32


@pytest.mark.gpu
def test_gi1_env_switch_keeps_the_torch_chain(golden_dir, monkeypatch):
    monkeypatch.setenv("FP8Q_GRAD_KERNELS", "0")
    calls = _spy(monkeypatch)
    _check_gi1(golden_dir)
    assert not calls
