"""The uniform (INT) quantizers against the REFERENCE (tests/golden/gu1_uniform.npz, written by
tests/golden/make_golden_uniform.py from the reference's QuantizationManager): after every one of three batches the
output, delta, zero_float and the symmetric sign -- per tensor and per channel, n_bits 2 / 4 / 8 / 16, the three min/max
estimators.  CPU: this repository's eager chain from the recorded ranges (the comparator of the kernel tests).  GPU: the
whole manager on the kernels, without a host round trip."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gu1_uniform.npz")
ESTS = ["current_minmax", "allminmax", "running_minmax"]
CASES = [(q, pc, nb) for q in ("sym", "asym") for pc in (0, 1) for nb in (2, 4, 8, 16)]


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _eq(got, want):
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float32)).reshape(-1)
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float32)).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _quantizer(qname, pc, nb):
    from quantization.uniform import SymmetricUniformQuantizer, AsymmetricUniformQuantizer
    return (SymmetricUniformQuantizer if qname == "sym" else AsymmetricUniformQuantizer)(n_bits=nb, per_channel=bool(pc))


@pytest.mark.parametrize("est", ESTS)
@pytest.mark.parametrize("qname,pc,nb", CASES)
def test_eager_chain_on_cpu_equals_the_reference(g, qname, pc, nb, est):
    key = f"{qname}_pc{pc}_b{nb}_{est}"
    xs = g[f"{qname}_pc{pc}_b{nb}_x"]
    q = _quantizer(qname, pc, nb)
    for i, x in enumerate(xs):
        xmin, xmax = torch.from_numpy(g[key + "_xmin"][i]), torch.from_numpy(g[key + "_xmax"][i])
        if not pc:
            xmin, xmax = xmin.reshape(()), xmax.reshape(())
        q.set_quant_range(xmin, xmax)
        y = q(torch.from_numpy(x))
        assert _eq(q.delta, g[key + "_delta"][i]), (key, i)
        if qname == "asym":
            assert _eq(q.zero_float, g[key + "_zf"][i]), (key, i)
        else:
            assert int(bool(q._signed)) == int(g[key + "_signed"][i]), (key, i)
        assert _eq(y, g[key + "_y"][i]), (key, i)


@pytest.mark.gpu
@pytest.mark.parametrize("est", ESTS)
@pytest.mark.parametrize("qname,pc,nb", CASES)
def test_kernels_equal_the_reference_without_a_sync(g, qname, pc, nb, est):
    from quantization.quantization_manager import QuantizationManager, QMethods
    from quantization.range_estimators import RangeEstimators
    key = f"{qname}_pc{pc}_b{nb}_{est}"
    xs = [torch.from_numpy(x).cuda() for x in g[f"{qname}_pc{pc}_b{nb}_x"]]
    qcls = QMethods.symmetric_uniform.cls if qname == "sym" else QMethods.asymmetric_uniform.cls

    def mk():
        return QuantizationManager(qmethod=qcls, init=RangeEstimators[est].cls, per_channel=bool(pc),
                                   qparams=dict(n_bits=nb))
    warm = mk()
    for x in xs:
        warm(x)
    qm = mk()
    rec = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for x in xs:
            y = qm(x)
            q = qm.quantizer
            rec.append((y.clone(), q.delta.clone(), None if qname == "sym" else q.zero_float.clone(),
                        q._signed.clone() if qname == "sym" else None))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for i, (y, d, zf, sg) in enumerate(rec):
        assert _eq(d.cpu().numpy(), g[key + "_delta"][i]), (key, i)
        if qname == "asym":
            assert _eq(zf.cpu().numpy(), g[key + "_zf"][i]), (key, i)
        else:
            assert sg.dtype == torch.bool and sg.dim() == 0
            assert int(bool(sg)) == int(g[key + "_signed"][i]), (key, i)
        assert _eq(y.cpu().numpy(), g[key + "_y"][i]), (key, i)
