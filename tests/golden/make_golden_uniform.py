#!/usr/bin/env python
"""Generate tests/golden/gu1_uniform.npz by IMPORTING the reference's uniform quantizers (a checkout of the reference
project is needed; run it where that checkout is, never from a test):

    python -B tests/golden/make_golden_uniform.py PATH_TO_REFERENCE_CHECKOUT

The reference's QuantizationManager with SymmetricUniformQuantizer / AsymmetricUniformQuantizer, per tensor and per
channel, n_bits in {2, 4, 8, 16}, current_minmax / allminmax / running_minmax over three batches (torch CPU, fp32).
Stored per case and batch: the input, the estimator's (xmin, xmax), delta, zero_float (asymmetric), signed (symmetric)
and the output.  The inputs hold exact ties (k + 0.5) * delta of the batch's own range, +-0, subnormals, values beyond
the range of later batches, an all-non-negative batch (the symmetric sign flips to unsigned), an all-non-positive one,
and (per channel) a channel with xmin == xmax == 0 and channels with +-inf / NaN.  Data only: nothing of the
reference's source is stored.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn

if len(sys.argv) != 2:
    raise SystemExit("usage: make_golden_uniform.py PATH_TO_REFERENCE_CHECKOUT")
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
from quantization.range_estimators import RangeEstimators  # noqa: E402
from quantization.quantization_manager import QuantizationManager, QMethods  # noqa: E402

torch.set_num_threads(1)

SHAPES = {0: (4, 6, 5, 5), 1: (6, 4, 5, 5)}
KINDS = ("signed", "nonneg", "nonpos")          # batch 0, 1, 2


def _delta_of(xmin, xmax, n_bits, sym):
    """the reference's delta for this batch's own range (fp32 torch ops, as set_quant_range)"""
    xmin = torch.min(xmin, torch.zeros_like(xmin))
    xmax = torch.max(xmax, torch.ones_like(xmax) * 1e-8)
    if sym:
        signed = bool(xmin.min() < 0)
        return torch.max(xmin.abs(), xmax) / (2.0 ** (n_bits - signed) - 1)
    return (xmax - xmin) / (2.0 ** n_bits - 1)


def make_batch(pc, kind, n_bits, sym, scale, g):
    shape = SHAPES[pc]
    C = shape[0] if pc else 1
    x = torch.randn(shape, generator=g) * scale
    if kind == "nonneg":
        x = x.abs()
    elif kind == "nonpos":
        x = -x.abs()
    rows = x.view(C, -1)
    # pin every row's range on its first two elements, then fill a third of the rest with exact ties of that range
    lo = -(torch.rand(C, generator=g) * scale + 0.5) if kind != "nonneg" else torch.rand(C, generator=g) * 0.1
    hi = (torch.rand(C, generator=g) * scale + 0.5) if kind != "nonpos" else -torch.rand(C, generator=g) * 0.1
    rows[:, 0], rows[:, 1] = lo, hi
    rows.clamp_(lo[:, None], hi[:, None])
    d = _delta_of(lo, hi, n_bits, sym).view(C, 1)
    n = rows.shape[1]
    k = torch.randint(-40, 40, (C, n), generator=g).float()
    if kind == "nonneg":
        k = k.abs()
    elif kind == "nonpos":
        k = -k.abs() - 1
    ties = ((k + 0.5) * d).clamp(lo[:, None], hi[:, None])
    m = torch.zeros(C, n, dtype=torch.bool)
    m[:, 2::3] = True
    rows[m] = ties[m]
    # +-0 and subnormals inside the range
    rows[:, 3] = 0.0
    rows[:, 4] = -0.0 if kind != "nonneg" else 0.0
    rows[:, 5] = 1e-40 if kind != "nonpos" else -1e-40
    rows[:, 7] = -1e-42 if kind != "nonneg" else 1e-42
    if pc:
        rows[1] = 0.0                                  # xmin == xmax == 0
        if kind == "signed":
            rows[2, 8] = float("inf")
            rows[3, 9] = float("-inf")
            rows[4, 10] = float("nan")
    return x


def make_gu1():
    out = {}
    ests = {"current_minmax": RangeEstimators.current_minmax.cls, "allminmax": RangeEstimators.allminmax.cls,
            "running_minmax": RangeEstimators.running_minmax.cls}
    qms = {"sym": QMethods.symmetric_uniform.cls, "asym": QMethods.asymmetric_uniform.cls}
    for qname, qcls in qms.items():
        for pc in (0, 1):
            for n_bits in (2, 4, 8, 16):
                g = torch.Generator().manual_seed(1000 * pc + n_bits + (7 if qname == "sym" else 0))
                xs = [make_batch(pc, kind, n_bits, qname == "sym", 1.0 + i, g) for i, kind in enumerate(KINDS)]
                if not pc:                     # later batches reach beyond the running / all-time range
                    xs[2].view(-1)[11] = -50.0
                out[f"{qname}_pc{pc}_b{n_bits}_x"] = np.stack([x.numpy() for x in xs])
                for ename, ecls in ests.items():
                    qm = QuantizationManager(qmethod=qcls, init=ecls, per_channel=bool(pc), qparams=dict(n_bits=n_bits))
                    rec = {k: [] for k in ("y", "xmin", "xmax", "delta", "zf", "signed")}
                    for x in xs:
                        y = qm(x)
                        q = qm.quantizer
                        rec["y"].append(y.detach().numpy().copy())
                        rec["xmin"].append(np.asarray(qm.range_estimator.current_xmin.detach().numpy(), np.float32).reshape(-1))
                        rec["xmax"].append(np.asarray(qm.range_estimator.current_xmax.detach().numpy(), np.float32).reshape(-1))
                        rec["delta"].append(q.delta.detach().numpy().copy().reshape(-1))
                        if qname == "asym":
                            rec["zf"].append(q.zero_float.detach().numpy().copy().reshape(-1))
                        else:
                            rec["signed"].append(int(bool(q._signed)))
                    key = f"{qname}_pc{pc}_b{n_bits}_{ename}"
                    for k, v in rec.items():
                        if v:
                            out[f"{key}_{k}"] = np.stack(v) if k != "signed" else np.array(v)
    path = os.path.join(OUT, "gu1_uniform.npz")
    np.savez_compressed(path, **out)
    print("gu1 ok", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make_gu1()
