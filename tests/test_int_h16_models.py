"""INT8 ResNet-18 and MobileNetV2 held in bfloat16 / float16 (keep_dtype=True on the uniform quantizers): calibrate one batch,
fix_ranges(), validate without a host synchronisation, and -- teacher-forced, so that nothing depends on whether the half
convolutions repeat bit for bit -- every QuantizationManager's output equals the float32 kernel on its own widened recorded
input, rounded once, and every calibrated range the float32 range kernels on its widened calibration input.  Without
keep_dtype the managers return float32, the values of the float32 route."""
import pytest
import torch

from test_models import _warm_bn
from test_int_h16_kernels import _same

pytestmark = pytest.mark.gpu

SIZE = 64


def _build(model, symmetric, keep_dtype):
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    qm = QMethods.symmetric_uniform.cls if symmetric else QMethods.asymmetric_uniform.cls
    kw = dict(method=qm, act_method=qm, weight_range_method=RangeEstimators.current_minmax.cls,
              act_range_method=RangeEstimators.running_minmax.cls, n_bits=8, n_bits_act=8, per_channel_weights=True)
    if keep_dtype:
        kw.update(act_quant_kwargs=dict(keep_dtype=True), weight_quant_kwargs=dict(keep_dtype=True))
    torch.manual_seed(0)
    if model == "r18":
        from models.resnet import resnet18
        from models.resnet_quantized import QuantizedResNet
        return QuantizedResNet(_warm_bn(resnet18()), input_size=(1, 3, SIZE, SIZE), **kw).eval()
    from models.mobilenet_v2 import MobileNetV2
    from models.mobilenet_v2_quantized import QuantizedMobileNetV2
    fp = _warm_bn(MobileNetV2(input_size=SIZE)).eval()
    return QuantizedMobileNetV2(fp, input_size=(1, 3, SIZE, SIZE), **kw).eval()


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


def _range_args(q):
    sym = q.symmetric
    return q._delta, None if sym else q._zero_float, q._signed if sym else None, q.n_bits, sym, q.eps


@pytest.mark.parametrize("model,dtype,symmetric", [("r18", torch.bfloat16, True), ("r18", torch.bfloat16, False),
                                                   ("mbv2", torch.bfloat16, True), ("mbv2", torch.bfloat16, False),
                                                   ("r18", torch.float16, True)])
def test_int8_half_model_calibrates_and_validates(model, dtype, symmetric, monkeypatch):
    from fp8q import ops
    monkeypatch.setenv("FP8Q_CACHE_WEIGHTS", "0")        # every manager runs in every forward
    g = torch.Generator().manual_seed(11)
    xc = torch.randn(8, 3, SIZE, SIZE, generator=g).cuda()
    xv = torch.randn(8, 3, SIZE, SIZE, generator=g).cuda()
    net = _build(model, symmetric, True).cuda().to(dtype)
    n_mgr = len(_managers(net))
    assert n_mgr > 20 and all(m.quantizer.keep_dtype for _, m in _managers(net))
    with torch.no_grad():
        net.set_quant_state(True, True)
        net.estimate_ranges()
        cal = []
        hs = _record(net, cal)
        net(xc.to(dtype))
        for h in hs:
            h.remove()
        net.fix_ranges()
        val = []
        hs = _record(net, val)
        xvd = xv.to(dtype)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            logits = net(xvd)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for h in hs:
            h.remove()
        assert logits.dtype == dtype and bool(torch.isfinite(logits.float()).all())

        # calibrated ranges: the float32 range kernels on the widened calibration input.  A manager that ran more than once in
        # the calibration pass (none does today) would hold the range of its last call; the check is for single calls.
        seen = {}
        for name, mgr, x, y in cal:
            seen[name] = (mgr, x)
        assert len(seen) == len(cal) and len(cal) > 20
        for name, (mgr, x) in seen.items():
            q = mgr.quantizer
            assert x.dtype == dtype, name
            if mgr.per_channel:
                w = ops.int_minmax_quantize(x.float(), 8, symmetric, q.eps)
                d, z, sg = w[3], w[4], w[5]
            else:
                mn, mx = ops.minmax(x.float(), False)
                d, z, sg = ops.int_set_range(mn, mx, 8, symmetric, q.eps)
            assert q._delta.dtype == torch.float32 and _same(q._delta.reshape(-1), d.reshape(-1)), name
            if symmetric:
                assert bool(q._signed) == bool(sg), name
            else:
                assert _same(q._zero_float.reshape(-1), z.reshape(-1)), name

        # validation outputs, teacher-forced: zero exemptions
        assert len(val) >= len(cal)
        for name, mgr, x, y in val:
            assert x.dtype == dtype and y.dtype == dtype, (name, x.dtype, y.dtype)
            want = ops.int_quantize(x.float(), *_range_args(mgr.quantizer)).to(dtype)
            assert _same(y, want), name

        # the same model without keep_dtype: every manager returns float32, the values of the float32 route -- what it
        # returned before the half lane existed (the manager widened with x.float())
        ref = _build(model, symmetric, False).cuda()
        ref.set_quant_state(True, True)
        ref.estimate_ranges()
        ref(xc)
        ref.fix_ranges()
        by_name = dict(_managers(ref))
        assert set(by_name) == {n for n, _ in _managers(net)}
        for name, _, x, _ in val:
            mgr = by_name[name]
            assert mgr.quantizer.keep_dtype is False
            y = mgr(x)
            assert y.dtype == torch.float32 and _same(y, mgr(x.float())), name
            assert _same(y, ops.int_quantize(x.float(), *_range_args(mgr.quantizer))), name
        out = ref(xv)
        assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
