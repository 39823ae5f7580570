#!/usr/bin/env python
"""Generate tests/golden/gh1_half.npz by IMPORTING the reference's FP8 quantizer and min/max estimators (a checkout of
the reference project is needed; run it where that checkout is, never from a test):

    python -B tests/golden/make_golden_h16.py PATH_TO_REFERENCE_CHECKOUT

The reference's quantize_to_fp8_ste_MM on float16 / bfloat16 tensors (torch CPU) with maxval and the mantissa width as
float32 tensors -- what its FPQuantizer holds -- per tensor and per channel, for (n_bits, M, sign_bits) in
{(8,2,1), (8,3,1), (8,4,1), (8,3,0), (6,2,1)}; and its Current / All / Running min/max estimators over three half
batches (as they are: the estimates have the input's dtype, the running fold is evaluated in it) and over the same
batches widened with .float() (estimates and fold in float32).  ATen's type promotion widens the half input and returns float32: the generator asserts that the output dtype
is float32 and that the result equals the same call on x.float(), and stores the float32 outputs.
Inputs are stored as uint16 bit patterns.  Every input holds a few thousand seeded elements plus the edge inputs: zeros
of both signs, subnormals, the largest finite value, infinities, NaN, and the exact rounding ties of every binade inside
the range that the input type can represent.  Data only: nothing of the reference's source is stored.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn

if len(sys.argv) != 2:
    raise SystemExit("usage: make_golden_h16.py PATH_TO_REFERENCE_CHECKOUT")
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
from quantization.range_estimators import RangeEstimators  # noqa: E402

torch.set_num_threads(1)

FORMATS = ((8, 2, 1), (8, 3, 1), (8, 4, 1), (8, 3, 0), (6, 2, 1))
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
C, INNER = 8, 512


def bits_of(x):
    return x.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def edge_values(dtype, maxval, M):
    """zeros, subnormals, extremes, non-finite values, and the ties (k + 1/2) * 2^(e - M) of every binade 2^e up to maxval"""
    fi = torch.finfo(dtype)
    v = [0.0, -0.0, fi.tiny, -fi.tiny, fi.tiny / 2, -fi.tiny / 4, fi.smallest_normal if hasattr(fi, "smallest_normal") else fi.tiny,
         fi.max, -fi.max, float("inf"), float("-inf"), float("nan"), maxval, -maxval, maxval * 1.5, 1.0, -1.0]
    top = int(np.floor(np.log2(maxval)))
    for e in range(top - 40, top + 1):
        step = 2.0 ** (e - M)
        for k in (2 ** M, 2 ** M + 1, 2 ** (M + 1) - 1):
            v += [(k + 0.5) * step, -(k + 0.5) * step]
    return torch.tensor(v, dtype=torch.float64).to(dtype)       # ties that the type cannot hold round to a neighbour: fine


def make_input(dtype, seed, maxval, M, pc):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(C, INNER, generator=g) * torch.exp(torch.randn(C, INNER, generator=g))).to(dtype)
    mv = (torch.rand(C, generator=g) * 2.0 + 0.05) * maxval if pc else torch.tensor([maxval])
    mv = mv.to(torch.float32)
    for c in range(C):
        e = edge_values(dtype, float(mv[c if pc else 0]), M)
        x[c, :e.numel()] = e[:INNER]
    return x, mv


def make_gh1():
    out = {}
    cases = []
    cid = 0
    for dname, dtype in DTYPES.items():
        for pc in (0, 1):
            for n_bits, M, s in FORMATS:
                for maxval in ((0.37, 448.0) if not pc else (1.0,)):
                    x, mv = make_input(dtype, 9000 + cid, maxval, M, pc)
                    mbits = torch.tensor([float(M)])
                    mvr = mv.view(C, 1) if pc else mv
                    y = quantize_to_fp8_ste_MM(x, n_bits, mvr, mbits, s)
                    y32 = quantize_to_fp8_ste_MM(x.float(), n_bits, mvr, mbits, s)
                    assert y.dtype == torch.float32, y.dtype
                    assert torch.equal(y.isnan(), y32.isnan()) and torch.equal(y.nan_to_num(0.0), y32.nan_to_num(0.0))
                    out[f"c{cid}_x"] = bits_of(x)
                    out[f"c{cid}_maxval"] = mv.numpy().copy()
                    out[f"c{cid}_y"] = y.numpy().copy()
                    cases.append((cid, 0 if dname == "f16" else 1, pc, n_bits, M, s))
                    cid += 1
    out["cases"] = np.array(cases, dtype=np.int64)

    # the three min/max estimators over three batches (the third reaches beyond the earlier ranges; signed zeros)
    ests = {"current_minmax": RangeEstimators.current_minmax.cls, "allminmax": RangeEstimators.allminmax.cls,
            "running_minmax": RangeEstimators.running_minmax.cls}
    for dname, dtype in DTYPES.items():
        for pc in (0, 1):
            g = torch.Generator().manual_seed(77 + pc)
            xs = [(torch.randn(C, 96, generator=g) * (1.0 + b)).to(dtype) for b in range(3)]
            xs[2][3, 5] = 40.0
            xs[1][2] = xs[1][2].abs()
            xs[1][2, 7] = 0.0
            out[f"mm_{dname}_pc{pc}_x"] = np.stack([bits_of(x) for x in xs])
            for ename, ecls in ests.items():
                est = ecls(per_channel=bool(pc))
                mins, maxs = [], []
                for x in xs:
                    mn, mx = est(x)
                    mins.append(np.asarray(mn.detach().float().numpy(), np.float32).reshape(-1))
                    maxs.append(np.asarray(mx.detach().float().numpy(), np.float32).reshape(-1))
                    out[f"mm_{dname}_pc{pc}_{ename}_dtype"] = np.array([str(mn.dtype)])
                out[f"mm_{dname}_pc{pc}_{ename}_min"] = np.stack(mins)
                out[f"mm_{dname}_pc{pc}_{ename}_max"] = np.stack(maxs)
                # the same estimator on the exactly widened batches: its fold runs in float32, which is what this project's
                # float32 running estimate has to equal bit for bit
                est = ecls(per_channel=bool(pc))
                mins, maxs = [], []
                for x in xs:
                    mn, mx = est(x.float())
                    assert mn.dtype == torch.float32
                    mins.append(np.asarray(mn.detach().numpy(), np.float32).reshape(-1))
                    maxs.append(np.asarray(mx.detach().numpy(), np.float32).reshape(-1))
                out[f"mm_{dname}_pc{pc}_{ename}_wmin"] = np.stack(mins)
                out[f"mm_{dname}_pc{pc}_{ename}_wmax"] = np.stack(maxs)
    path = os.path.join(OUT, "gh1_half.npz")
    np.savez_compressed(path, **out)
    print("gh1 ok", os.path.getsize(path), "bytes", cid, "cases")


if __name__ == "__main__":
    make_gh1()
