"""ResNet-18 and MobileNetV2 held in bfloat16 / float16 (keep_dtype=True): calibrate, fix_ranges(), validate without a
host synchronisation, and -- teacher-forced, so that nothing depends on whether the half convolutions repeat bit for
bit -- every QuantizationManager's output equals the oracle on its own recorded input, every calibrated range the
oracle's min/max of its recorded calibration input."""
import copy

import numpy as np
import pytest
import torch

import oracle
from test_models import _warm_bn

pytestmark = pytest.mark.gpu

SIZE = 64


def _qparams(M, keep_dtype=True, w_est="current_minmax", a_est="allminmax"):
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    return dict(method=QMethods.fp_quantizer.cls, weight_range_method=RangeEstimators[w_est].cls,
                act_range_method=RangeEstimators[a_est].cls, n_bits=8, n_bits_act=8, per_channel_weights=True,
                fp8_kwargs=dict(maxval=None, mantissa_bits=M, set_maxval=True, keep_dtype=keep_dtype))


def _build(model, M):
    torch.manual_seed(0)
    if model == "r18":
        from models.resnet import resnet18
        from models.resnet_quantized import QuantizedResNet
        return QuantizedResNet(_warm_bn(resnet18()), input_size=(1, 3, SIZE, SIZE), **_qparams(M)).eval()
    from models.mobilenet_v2 import MobileNetV2
    from models.mobilenet_v2_quantized import QuantizedMobileNetV2
    fp = _warm_bn(MobileNetV2(input_size=SIZE)).eval()
    return QuantizedMobileNetV2(fp, input_size=(1, 3, SIZE, SIZE), **_qparams(M)).eval()


def _managers(net):
    from quantization.manager import QuantizationManager
    return [(n, m) for n, m in net.named_modules() if isinstance(m, QuantizationManager)]


def _record(net, log):
    """forward hooks that keep device copies of every manager's input and output (no host round trip)"""
    hs = []
    for name, m in _managers(net):
        def hook(mod, args, out, name=name):
            log.append((name, mod, args[0].detach().clone(), out.detach().clone()))
        hs.append(m.register_forward_hook(hook))
    return hs


def _same_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(np.int32 if a.itemsize == 4 else np.int16),
                                                                            np.where(nb, 0, b).view(np.int32 if b.itemsize == 4 else np.int16))


def _oracle_out(x, q, pc):
    xf = x.float().cpu().contiguous()
    mv = q.maxval.detach().float().cpu().reshape(-1)
    x2 = xf.reshape(xf.shape[0], -1) if pc else xf.reshape(1, -1)
    y = oracle.c_quantize(x2.numpy(), mv.numpy(), float(q.mantissa_bits), q.n_bits, q.sign_bits)
    return torch.from_numpy(y).view(xf.shape)


@pytest.mark.parametrize("model,dtype,M", [("r18", torch.bfloat16, 3), ("r18", torch.bfloat16, 2), ("r18", torch.float16, 3),
                                           ("r18", torch.float16, 2), ("mbv2", torch.bfloat16, 3), ("mbv2", torch.bfloat16, 2)])
def test_half_model_calibrates_and_validates(model, dtype, M, monkeypatch):
    # every manager runs in every forward, in the fp32 copy too (no cached / pre-quantized weights, no fused epilogue that
    # would bypass the managers' forward): the settings under which the two counts are comparable
    monkeypatch.setenv("FP8Q_CACHE_WEIGHTS", "0")
    monkeypatch.setenv("FP8Q_FUSE_EPILOGUE", "0")
    g = torch.Generator().manual_seed(11)
    xc = torch.randn(8, 3, SIZE, SIZE, generator=g)
    xv = torch.randn(8, 3, SIZE, SIZE, generator=g)

    net32 = _build(model, M).cuda()
    net = copy.deepcopy(net32).to(dtype)
    with torch.no_grad():
        # the fp32 copy: how many managers run in a validation pass
        net32.set_quant_state(True, True)
        net32.estimate_ranges()
        net32(xc.cuda())
        net32.fix_ranges()
        log32 = []
        hs = _record(net32, log32)
        net32(xv.cuda())
        for h in hs:
            h.remove()
        n_expected = len(log32)
        assert n_expected > 20

        net.set_quant_state(True, True)
        net.estimate_ranges()
        cal = []
        hs = _record(net, cal)
        net(xc.cuda().to(dtype))
        for h in hs:
            h.remove()
        net.fix_ranges()
        val = []
        hs = _record(net, val)
        xvd = xv.cuda().to(dtype)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            logits = net(xvd)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for h in hs:
            h.remove()
    assert logits.dtype == dtype and bool(torch.isfinite(logits.float()).all())

    # calibrated ranges: the oracle's min/max of the recorded calibration input (per channel for weights)
    seen = {}
    for name, mgr, x, y in cal:
        seen[name] = (mgr, x)
    assert len(seen) == len(cal)
    for name, (mgr, x) in seen.items():
        pc = mgr.per_channel
        xf = x.float().cpu().contiguous().numpy()
        mn, mx = oracle.c_minmax(xf.reshape(xf.shape[0], -1) if pc else xf.reshape(1, -1), True)
        est = mgr.range_estimator
        assert _same_nan(est.current_xmin.detach().cpu().numpy().reshape(-1), mn), name
        assert _same_nan(est.current_xmax.detach().cpu().numpy().reshape(-1), mx), name
        assert _same_nan(mgr.quantizer.maxval.detach().cpu().numpy().reshape(-1), oracle.c_absmax(mn, mx)), name
        assert mgr.quantizer.maxval.dtype == torch.float32

    # validation outputs, teacher-forced: zero exemptions
    checked = 0
    for name, mgr, x, y in val:
        assert x.dtype == dtype and y.dtype == dtype, (name, x.dtype, y.dtype)
        want = _oracle_out(x, mgr.quantizer, mgr.per_channel).to(dtype)
        assert _nan_tolerant_equal(y.cpu(), want), name
        checked += 1
    assert checked == n_expected, (checked, n_expected)


def _nan_tolerant_equal(a, b):
    """equal bit patterns, except that a NaN matches any NaN"""
    if not torch.equal(a.isnan(), b.isnan()):
        return False
    return torch.equal(a.nan_to_num(0.0).contiguous().view(torch.int16), b.nan_to_num(0.0).contiguous().view(torch.int16))


def test_keep_dtype_false_returns_fp32():
    from quantization.fp8 import FPQuantizer
    q = FPQuantizer(n_bits=8, mantissa_bits=3, maxval=1.7, set_maxval=True).cuda()
    x = (torch.randn(4, 33, 5, generator=torch.Generator().manual_seed(2)) * 2).to(torch.bfloat16)
    with torch.no_grad():
        y = q(x.cuda())
    assert y.dtype == torch.float32
    want = _oracle_out(x, q, False)
    assert _same_nan(y.cpu().numpy(), want.numpy())
    q.keep_dtype = True
    with torch.no_grad():
        yh = q(x.cuda())
    assert yh.dtype == torch.bfloat16 and _nan_tolerant_equal(yh.cpu(), want.to(torch.bfloat16))
    # under autograd the input is widened and takes the fp32 route (straight-through gradient)
    q.keep_dtype = False
    xg = x.cuda().requires_grad_(True)
    yg = q(xg)
    assert yg.dtype == torch.float32 and _same_nan(yg.detach().cpu().numpy(), want.numpy())
    yg.sum().backward()
    assert xg.grad is not None and xg.grad.dtype == torch.bfloat16


def test_mse_estimator_falls_back_on_half_input():
    """the MSE search is float32-only: a bf16 input is widened, same range and output as the fp32 estimator on x.float()"""
    from quantization.manager import QuantizationManager
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    x = (torch.randn(8, 16, 12, 12, generator=torch.Generator().manual_seed(4)) * 1.3).to(torch.bfloat16)

    def make(keep):
        return QuantizationManager(qmethod=QMethods.fp_quantizer.cls, init=RangeEstimators.MSE.cls, per_channel=False,
                                   qparams=dict(n_bits=8, mantissa_bits=3, set_maxval=True, maxval=None,
                                                mse_include_mantissa_bits=False, keep_dtype=keep)).cuda()
    a, b = make(True), make(False)
    with torch.no_grad():
        ya = a(x.cuda())
        yb = b(x.float().cuda())
    assert ya.dtype == torch.bfloat16 and yb.dtype == torch.float32
    assert _same_nan(a.quantizer.maxval.cpu().numpy(), b.quantizer.maxval.cpu().numpy())
    assert float(a.quantizer.mantissa_bits) == float(b.quantizer.mantissa_bits)
    assert _nan_tolerant_equal(ya.cpu(), yb.cpu().to(torch.bfloat16))
