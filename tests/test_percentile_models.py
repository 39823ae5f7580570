"""CurrentMinMaxEstimator(percentile=p) through the operator API: CUDA float32 / half inputs take the selection kernels
(fp8q.ops.percentile), any size; FP8Q_PERCENTILE_KERNELS=0 keeps torch.quantile."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from percentile_oracle import Oracle, assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_per_tensor_estimate_of_a_tensor_torch_quantile_refuses():
    """2^24 + 1 elements: torch.quantile raises "input tensor is too large"; the selection kernels have no such limit"""
    from quantization.range_estimators import CurrentMinMaxEstimator
    n = (1 << 24) + 1
    x_np = np.random.RandomState(11).randn(n).astype(np.float32)
    est = CurrentMinMaxEstimator(percentile=0.1, per_channel=False)
    lo, hi = est(torch.from_numpy(x_np).cuda())
    assert lo.shape == hi.shape == () and lo.dtype == torch.float32
    assert est.current_xmin is lo and est.current_xmax is hi and est.last_maxval is None
    wlo, whi = Oracle(x_np.reshape(1, -1)).ranges(0.1)
    assert_bits(lo.cpu().numpy(), wlo)
    assert_bits(hi.cpu().numpy(), whi)


def test_per_channel_estimate_and_a_bfloat16_input():
    from quantization.range_estimators import CurrentMinMaxEstimator
    x_np = np.random.RandomState(12).randn(64, 3, 7, 7).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    est = CurrentMinMaxEstimator(percentile=1.0, per_channel=True)
    lo, hi = est(x)
    assert lo.shape == hi.shape == (64,)
    wlo, whi = Oracle(x_np.reshape(64, -1)).ranges(1.0)
    assert_bits(lo.cpu().numpy(), wlo)
    assert_bits(hi.cpu().numpy(), whi)
    xb = x.to(torch.bfloat16)
    blo, bhi = CurrentMinMaxEstimator(percentile=1.0, per_channel=True)(xb)
    assert blo.dtype == torch.float32 and bhi.dtype == torch.float32
    wlo, whi = Oracle(xb.float().cpu().numpy().reshape(64, -1)).ranges(1.0)
    assert_bits(blo.cpu().numpy(), wlo)
    assert_bits(bhi.cpu().numpy(), whi)


_CHILD = r"""
import sys
import numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from quantization.range_estimators import CurrentMinMaxEstimator
import fp8q
called = []
fp8q.ops.percentile = lambda *a, **k: called.append(1)
x = torch.from_numpy(np.random.RandomState(5).randn(48, 300).astype(np.float32)).cuda()
for pc in (False, True):
    lo, hi = CurrentMinMaxEstimator(percentile=1.0, per_channel=pc)(x)
    f = x.reshape(48, -1) if pc else x.reshape(-1)
    q = torch.tensor([1.0 / 100.0, 1 - 1.0 / 100.0], device=x.device, dtype=torch.float64)
    wlo, whi = torch.quantile(f.double(), q, dim=-1).float()
    assert lo.shape == wlo.shape and torch.equal(lo, wlo) and torch.equal(hi, whi), pc
assert not called
print("quantile-branch-ok")
"""


def test_the_environment_switch_keeps_the_torch_quantile_branch():
    env = dict(os.environ, FP8Q_PERCENTILE_KERNELS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "fp8-quantization_amd")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "quantile-branch-ok" in r.stdout, r.stdout + r.stderr


def test_quantization_manager_with_a_percentile_range_and_its_deepcopy():
    from quantization.quantizers.fp8_quantizer import FPQuantizer
    from quantization.range_estimators import RangeEstimators
    from quantization.quantization_manager import QuantizationManager
    import fp8q
    x_np = np.random.RandomState(13).randn(64, 32, 28, 28).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    mgr = QuantizationManager(qmethod=FPQuantizer, init=RangeEstimators.current_minmax.cls, per_channel=False,
                              qparams=dict(n_bits=8, mantissa_bits=3, set_maxval=True),
                              range_estim_params=dict(percentile=1.0))
    mgr.estimate_ranges()
    y = mgr(x)
    wlo, whi = Oracle(x_np.reshape(1, -1)).ranges(1.0)
    want_mv = np.maximum(np.abs(wlo), np.abs(whi)).astype(np.float32)
    assert_bits(mgr.range_estimator.current_xmin.cpu().numpy(), wlo)
    assert_bits(mgr.range_estimator.current_xmax.cpu().numpy(), whi)
    assert_bits(mgr.quantizer.maxval.detach().cpu().numpy(), want_mv)
    want = fp8q.ops.quantize(x, torch.from_numpy(want_mv).cuda(), 3.0, 8, 1)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    twin = copy.deepcopy(mgr)                                   # nothing native is kept on the estimator
    assert torch.equal(twin.range_estimator.current_xmin, mgr.range_estimator.current_xmin)
    assert torch.equal(twin(x).view(torch.int32), y.view(torch.int32))
