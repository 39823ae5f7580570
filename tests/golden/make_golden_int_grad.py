#!/usr/bin/env python
"""Generate tests/golden/gi1_int_grad.npz by IMPORTING the reference's two uniform quantizers and running their CPU autograd
(a checkout of the reference project is needed; run it where that checkout is, never from a test):

    python -B tests/golden/make_golden_int_grad.py PATH_TO_REFERENCE_CHECKOUT

Per case: set_quant_range (about 0.7 x the data's min / max, so both ends clip), one forward without autograd (it brings a
per-channel delta into the input's rank, which the reference can only do while delta is still a buffer),
make_range_trainable, forward, backward on the CPU.
Layouts, at shapes the models meet: [64,3,7,7] per channel and per tensor (the same x and g), [96,1,3,3] per channel (rows of
9), [8,32,14,14] per tensor, [5,1031] per channel.  On every layout: {asymmetric, symmetric signed, symmetric one-sided
(x_min = 0: the unsigned grid)} x n_bits {8, 4} x grad_scaling {off, on} -- 60 cases, none left out.
Every row holds elements exactly on both ends of its integer grid, an exact half-step tie and +-0; the upstream gradient has
zeros and no nonzero entry below 1e-20, so the reference's g * scale stays normal.
Stored: x and g per shape and, per layout, kind and n_bits, the five leading elements of every row that replace x's there
(`xs_...`: they depend on the case's grid); per case delta, zero_float, the sign, gdelta, gzero_float and gx -- the latter as the XOR of its
bits with those of g * m (m the 0 / 1 mask of include/fp8q.h, formed here in numpy), which is almost everywhere 0 or 1 and
compresses well; cases whose XOR array is the same to the bit share one stored array `gxx_<index>`.
Also printed: MEASURED_RATIO for tests/test_int_grad_golden.py.
Data only: nothing of the reference's source is stored.
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn

if len(sys.argv) != 2:
    raise SystemExit("usage: make_golden_int_grad.py PATH_TO_REFERENCE_CHECKOUT")
REF = os.path.abspath(sys.argv[1])
OUT = os.path.dirname(os.path.abspath(__file__))


def _install_stubs():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    mk = lambda n: type(n, (nn.Module,), {})
    stub("timm")
    stub("timm.models")
    stub("timm.models.layers")
    stub("timm.models.layers.activations", Swish=mk("Swish"), HardSwish=mk("HardSwish"),
         HardSigmoid=mk("HardSigmoid"))
    stub("timm.models.layers.activations_me", SwishMe=mk("SwishMe"), HardSwishMe=mk("HardSwishMe"),
         HardSigmoidMe=mk("HardSigmoidMe"))


_install_stubs()
sys.path.insert(0, REF)
from quantization.quantizers.uniform_quantizers import AsymmetricUniformQuantizer, SymmetricUniformQuantizer  # noqa: E402

torch.set_num_threads(1)
F32 = np.float32
EPS = 1e-8

SHAPES = {"w7": (64, 3, 7, 7), "dw": (96, 1, 3, 3), "act": (8, 32, 14, 14), "odd": (5, 1031)}
LAYOUTS = [("w7_pc", "w7", 1), ("w7_pt", "w7", 0), ("dw_pc", "dw", 1), ("act_pt", "act", 0), ("odd_pc", "odd", 1)]
KINDS = ("asym", "sym_signed", "sym_onesided")


def contract(x, g, delta, zf, signed, n_bits, kind):
    """include/fp8q.h in numpy: g * m, and per row the float64 sums of the fp32 terms and of their magnitudes (masks applied)"""
    C = delta.size
    sym = kind != "asym"
    lo, hi = (F32(-2.0 ** (n_bits - 1)), F32(2.0 ** (n_bits - 1) - 1)) if (sym and signed) else (F32(0), F32(2.0 ** n_bits - 1))
    xr, gr = x.reshape(C, -1), g.reshape(C, -1)
    scale = np.maximum(delta, F32(EPS)).reshape(C, 1)
    zp = np.zeros((C, 1), F32) if sym else np.clip(np.rint(zf), lo, hi).reshape(C, 1)
    t = xr / scale
    u = np.rint(t) + zp
    m = ((u >= lo) & (u <= hi)).astype(F32)
    w = (np.clip(u, lo, hi) - zp) - m * t
    ta, tb = gr * w, (F32(1) - m) * (gr * scale)
    assert ta.dtype == np.float32 and tb.dtype == np.float32
    sa, abs_a = ta.astype(np.float64).sum(1), np.abs(ta).astype(np.float64).sum(1)
    sb, abs_b = -tb.astype(np.float64).sum(1), np.abs(tb).astype(np.float64).sum(1)
    sa = np.where(delta >= F32(EPS), sa, 0.0)
    if not sym:
        rz = np.rint(zf)
        sb = np.where((rz >= lo) & (rz <= hi), sb, 0.0)
    return (gr * m).reshape(x.shape), sa, abs_a, sb, abs_b, float(hi)


def ratio(diff, mag):
    """largest |diff| / mag; a row without terms (mag == 0) must agree exactly"""
    diff = np.abs(diff)
    assert (diff[mag == 0] == 0).all()
    return float((diff[mag > 0] / mag[mag > 0]).max()) if (mag > 0).any() else 0.0


def ranges(rows, kind):
    mn, mx = F32(0.7) * rows.min(1), F32(0.7) * rows.max(1)
    if kind == "sym_onesided":
        mn = np.zeros_like(mn)
    return torch.from_numpy(mn.astype(F32)), torch.from_numpy(mx.astype(F32))


def make_gi1():
    out, cases, stored = {}, [], {}
    rng = np.random.RandomState(2121)
    for sid, shape in SHAPES.items():
        out[f"x_{sid}"] = (rng.randn(*shape) * 0.8).astype(F32)
        g = rng.randn(*shape).astype(F32)
        g[np.abs(g) < 1e-20] = 0.0
        g.reshape(shape[0], -1)[:, 6] = 0.0
        out[f"g_{sid}"] = g
    worst = 0.0
    for lid, sid, pc in LAYOUTS:
        shape = SHAPES[sid]
        C = shape[0] if pc else 1
        for kind in KINDS:
            for n_bits in (8, 4):
                cls = AsymmetricUniformQuantizer if kind == "asym" else SymmetricUniformQuantizer
                # the case's own x: the shape's data with every row's grid ends, a tie and +-0 written in
                x = out[f"x_{sid}"].copy()
                rows = x.reshape(C, -1)
                probe = cls(n_bits=n_bits, per_channel=bool(pc))
                probe.set_quant_range(*ranges(rows, kind))
                scale = np.maximum(probe.delta.numpy().reshape(C), F32(EPS))
                zp = np.zeros(C, F32) if kind != "asym" else probe.zero_point.numpy().reshape(C)
                rows[:, 0] = scale * (F32(probe.int_min) - zp)
                rows[:, 1] = scale * (F32(probe.int_max) - zp)
                rows[:, 2] = F32(1.5) * scale
                rows[:, 3], rows[:, 4] = 0.0, -0.0
                xkey = f"xs_{lid}_{kind}_b{n_bits}"
                out[xkey] = rows[:, :5].copy()
                g = out[f"g_{sid}"]
                for gs in (0, 1):
                    k = len(cases)
                    q = cls(n_bits=n_bits, per_channel=bool(pc), grad_scaling=bool(gs))
                    q.set_quant_range(*ranges(out[f"x_{sid}"].reshape(C, -1), kind))
                    xt = torch.from_numpy(x.copy())
                    with torch.no_grad():
                        q(xt)
                    q.make_range_trainable()
                    xt.requires_grad_(True)
                    y = q(xt)
                    y.backward(torch.from_numpy(g))
                    delta = q._delta.detach().numpy().reshape(-1).copy()
                    zf = q._zero_float.detach().numpy().reshape(-1).copy() if kind == "asym" else None
                    signed = int(bool(q._signed)) if kind != "asym" else 0
                    assert signed == (kind == "sym_signed")
                    gd = q._delta.grad.numpy().reshape(-1).copy()
                    gz = q._zero_float.grad.numpy().reshape(-1).copy() if kind == "asym" else None
                    gx = xt.grad.numpy()
                    base, sa, abs_a, sb, abs_b, hi = contract(x, g, delta, zf, signed, n_bits, kind)
                    n_el = x.size // shape[0] if pc else x.size
                    f = float(F32(1.0 / np.sqrt(hi * n_el))) if gs else 1.0
                    ra = ratio(f * sa - gd, f * abs_a)
                    rb = ratio(f * sb - gz, f * abs_b) if gz is not None else 0.0
                    worst = max(worst, ra, rb)
                    assert np.array_equal(gx == 0, base == 0), (lid, kind, n_bits)
                    xor = gx.view(np.uint32) ^ base.view(np.uint32)
                    key = xor.tobytes()
                    if key not in stored:
                        stored[key] = len(stored)
                        out[f"gxx_{stored[key]}"] = xor
                    out[f"c{k}_delta"], out[f"c{k}_gdelta"] = delta, gd
                    if zf is not None:
                        out[f"c{k}_zf"], out[f"c{k}_gzf"] = zf, gz
                    cases.append(dict(k=k, layout=lid, shape=sid, x=xkey, per_channel=pc, kind=kind, n_bits=n_bits,
                                      signed=signed, grad_scaling=gs, gx=stored[key]))
                    print(f"{lid} {kind} b{n_bits} gs{gs}: gdelta {ra:.3e} gzero_float {rb:.3e} of the sums of magnitudes")
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(OUT, "gi1_int_grad.npz")
    np.savez_compressed(path, **out)
    print("gi1:", len(cases), "cases,", len(stored), "gx arrays,", os.path.getsize(path), "bytes")
    print(f"MEASURED_RATIO = {worst:.3e}")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    make_gi1()
