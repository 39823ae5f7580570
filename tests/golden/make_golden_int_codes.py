#!/usr/bin/env python
"""Generate tests/golden/gu2_uniform_int.npz by IMPORTING the reference's uniform quantizers (a checkout of the reference
project is needed; run it where that checkout is, never from a test):

    python -B tests/golden/make_golden_int_codes.py PATH_TO_REFERENCE_CHECKOUT

For every case of gu1_uniform.npz (symmetric / asymmetric x per tensor / per channel x n_bits 2, 4, 8, 16 x three batches)
the reference's quantizer gets set_quant_range(xmin, xmax) of that case's `current_minmax` record and the float32 tensor of
integers its to_integer_forward(x) returns is stored under `<case>_t` ([3, *shape]).  The inputs are NOT stored again: they
are gu1's `<case>_x`, read from gu1_uniform.npz by key (as are the ranges).  Data only: nothing of the reference's source is
stored.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn

if len(sys.argv) != 2:
    raise SystemExit("usage: make_golden_int_codes.py PATH_TO_REFERENCE_CHECKOUT")
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
from quantization.quantization_manager import QMethods  # noqa: E402

torch.set_num_threads(1)


def make_gu2():
    gu1 = np.load(os.path.join(OUT, "gu1_uniform.npz"))
    qms = {"sym": QMethods.symmetric_uniform.cls, "asym": QMethods.asymmetric_uniform.cls}
    out = {}
    for qname, qcls in qms.items():
        for pc in (0, 1):
            for n_bits in (2, 4, 8, 16):
                case = f"{qname}_pc{pc}_b{n_bits}"
                rec = f"{case}_current_minmax"
                ts = []
                for i, x in enumerate(gu1[f"{case}_x"]):
                    xmin, xmax = torch.from_numpy(gu1[rec + "_xmin"][i]), torch.from_numpy(gu1[rec + "_xmax"][i])
                    if not pc:
                        xmin, xmax = xmin.reshape(()), xmax.reshape(())
                    q = qcls(n_bits=n_bits, per_channel=bool(pc))
                    q.set_quant_range(xmin, xmax)
                    # the ranges are the recorded ones: the integers below belong to gu1's delta / zf / signed
                    assert np.array_equal(q.delta.detach().numpy().reshape(-1).view(np.int32),
                                          gu1[rec + "_delta"][i].view(np.int32)), (case, i)
                    xt = torch.from_numpy(x)
                    if pc:
                        q._adjust_params_per_channel(xt)      # the reference's forward does this before to_integer_forward
                    t = q.to_integer_forward(xt)
                    ts.append(t.detach().numpy().astype(np.float32, copy=True))
                out[f"{case}_t"] = np.stack(ts)
    path = os.path.join(OUT, "gu2_uniform_int.npz")
    np.savez_compressed(path, **out)
    print("gu2 ok", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make_gu2()
