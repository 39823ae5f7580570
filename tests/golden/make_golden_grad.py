#!/usr/bin/env python
"""Generate tests/golden/g14_grad.npz by IMPORTING the reference's quantize_to_fp8_ste_MM and running its CPU autograd (a
checkout of the reference project is needed; run it where that checkout is, never from a test):

    python -B tests/golden/make_golden_grad.py PATH_TO_REFERENCE_CHECKOUT

Layouts, at shapes the models meet: [64,3,7,7] per channel and per tensor (the same x and g), [96,1,3,3] per channel (rows of
9), [8,32,14,14] per tensor, [5,1031] per channel.  Formats, all of them on every layout: n_bits 8 and 6, widths 1..5 and the
non-integer 2.5, sign_bits 1 and 0 -- 24 formats, 120 cases, E = 0 (n_bits 6, signed, width 5) and E = 7 (n_bits 8, unsigned,
width 1) included.
Every row holds elements exactly on +maxval, on -maxval and at 0 (the lower bound of the unsigned formats).
Stored: x and g per shape, maxval per layout; per case gmaxval, gmbits and gx -- the latter as the XOR of its bits with those
of g * m (m the 0 / 0.5 / 1 mask, formed here in numpy), which is almost everywhere 0 or 1 and compresses well.  Cases of one
layout whose gx is the same array to the bit (width 2.5 rounds to 2; n_bits 8 and 6 at the same width differ by a power of two
in every scale) share one stored XOR array: a case's "gx" entry is the index of its array `gxx_<index>`.
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
    raise SystemExit("usage: make_golden_grad.py PATH_TO_REFERENCE_CHECKOUT")
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
from quantization.quantizers.fp8_quantizer import quantize_to_fp8_ste_MM  # noqa: E402

torch.set_num_threads(1)

SHAPES = {"w7": (64, 3, 7, 7), "dw": (96, 1, 3, 3), "act": (8, 32, 14, 14), "odd": (5, 1031)}
LAYOUTS = [("w7_pc", "w7", 1), ("w7_pt", "w7", 0), ("dw_pc", "dw", 1), ("act_pt", "act", 0), ("odd_pc", "odd", 1)]
WIDTHS = (1.0, 2.0, 3.0, 4.0, 5.0, 2.5)
ALL_FORMATS = [(nb, mb, sb) for nb in (8, 6) for sb in (1, 0) for mb in WIDTHS]
PT_MAXVAL = np.float32(1.3)


def mask_times_g(x, g, mv, sign_bits):
    """g * m in fp32, m = 1 inside (lo, maxval), 0.5 on a bound, 0 outside; mv broadcastable to x"""
    lo = -mv if sign_bits == 1 else np.zeros_like(mv)
    with np.errstate(invalid="ignore"):
        m = ((x > lo) & (x < mv)).astype(np.float32) + np.float32(0.5) * ((x == mv) | (x == lo)).astype(np.float32)
        return (g * m).astype(np.float32)


def make_g14():
    out, cases, stored = {}, [], {}
    rng = np.random.RandomState(1414)
    mvs = {}
    for sid, shape in SHAPES.items():
        C = shape[0]
        x = (rng.randn(*shape) * 0.8).astype(np.float32)
        rows = x.reshape(C, -1)
        mv_pc = (np.abs(rng.randn(C)) + 0.3).astype(np.float32)
        # exactly on the bounds of both channel modes, and at 0 (-0 too)
        rows[:, 0], rows[:, 1], rows[:, 2] = mv_pc, -mv_pc, 0.0
        rows[:, 3], rows[:, 4], rows[:, 5] = PT_MAXVAL, -PT_MAXVAL, -0.0
        out[f"x_{sid}"] = x
        out[f"g_{sid}"] = rng.randn(*shape).astype(np.float32)
        mvs[sid] = mv_pc
    for lid, sid, pc in LAYOUTS:
        mv = mvs[sid] if pc else np.array([PT_MAXVAL], np.float32)
        out[f"maxval_{lid}"] = mv
        x, g = out[f"x_{sid}"], out[f"g_{sid}"]
        for n_bits, mb, sb in ALL_FORMATS:
            k = len(cases)
            xt = torch.from_numpy(x.copy()).requires_grad_(True)
            mt = torch.from_numpy(mv.copy()).requires_grad_(True)
            bt = torch.Tensor([mb]).requires_grad_(True)
            y = quantize_to_fp8_ste_MM(xt, n_bits, mt, bt, sb)
            y.backward(torch.from_numpy(g))
            gx = xt.grad.numpy()
            mvb = mv.reshape([-1] + [1] * (x.ndim - 1)) if pc else mv
            base = mask_times_g(x, g, mvb, sb)
            xor = gx.view(np.uint32) ^ base.view(np.uint32)
            assert np.array_equal((xor ^ base.view(np.uint32)), gx.view(np.uint32))
            key = (lid, xor.tobytes())
            if key not in stored:
                stored[key] = len(stored)
                out[f"gxx_{stored[key]}"] = xor
            out[f"c{k}_gmaxval"] = mt.grad.numpy().copy()
            out[f"c{k}_gmbits"] = bt.grad.numpy().copy()
            cases.append(dict(k=k, layout=lid, shape=sid, per_channel=pc, n_bits=n_bits, mbits=mb, sign_bits=sb, gx=stored[key]))
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(OUT, "g14_grad.npz")
    np.savez_compressed(path, **out)
    print("g14:", len(cases), "cases,", len(stored), "gx arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    make_g14()
