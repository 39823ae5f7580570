"""The FP quantizer's backward where the models use it: a quantizer step with learned maxval and mantissa width that never
synchronises, and every _FakeQuantSTE call of one ResNet-18 / MobileNetV2 backward (learn_ranges state, learn_maxval,
per-channel weights, per-tensor activations) replayed through the kernel and through the torch chain.

End-to-end parameter gradients are NOT compared across the routes: convolution backward is not bit-reproducible."""
import numpy as np
import pytest
import torch

from test_grad_kernels import BOUND, _bits, _chain, _host_sums
from test_models import _managers, _warm_bn
from test_teacher_forced import N_CALLS

pytestmark = pytest.mark.gpu


def test_quantizer_step_with_learned_ranges_is_sync_free():
    from quantization.fp8 import FPQuantizer
    q = FPQuantizer(n_bits=8, mantissa_bits=3, maxval=1.5)
    q.maxval = q.maxval.cuda()
    q.learn_maxval()
    q.learn_mantissa_bits()
    assert q.maxval.is_cuda and q.mantissa_bits.is_cuda
    torch.manual_seed(3)
    x = (torch.randn(16, 64, device="cuda") * 2).requires_grad_(True)
    q(x).sum().backward()                        # library load, workspace allocation
    q.maxval.grad = q.mantissa_bits.grad = x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        q(x).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for p in (q.maxval, q.mantissa_bits):
        assert p.grad is not None and p.grad.device == p.device and p.grad.dtype == p.dtype
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
    assert x.grad is not None and float(x.grad.abs().sum()) > 0


def _build(tag):
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    qparams = dict(method=QMethods.fp_quantizer.cls, weight_range_method=RangeEstimators.current_minmax.cls,
                   act_range_method=RangeEstimators.allminmax.cls, n_bits=8, n_bits_act=8, per_channel_weights=True,
                   fp8_kwargs=dict(maxval=None, mantissa_bits=2 if tag == "r18" else 3, set_maxval=True, learn_maxval=True,
                                   learn_mantissa_bits=False, mse_include_mantissa_bits=False, allow_unsigned=False))
    torch.manual_seed(0)
    if tag == "r18":
        from models.resnet import resnet18
        from models.resnet_quantized import QuantizedResNet
        return QuantizedResNet(_warm_bn(resnet18(pretrained=False)), input_size=(1, 3, 64, 64), **qparams).eval()
    from models.mobilenet_v2 import MobileNetV2
    from models.mobilenet_v2_quantized import QuantizedMobileNetV2
    return QuantizedMobileNetV2(_warm_bn(MobileNetV2(input_size=64)), input_size=(1, 3, 64, 64), **qparams).eval()


@pytest.mark.parametrize("tag", ["r18", "mbv2"])
def test_every_quantizer_backward_of_a_model(tag, monkeypatch):
    from fp8q import ops
    from quantization.fp8 import FPQuantizer
    q = _build(tag).cuda()
    torch.manual_seed(5)
    batch = torch.randn(8, 3, 64, 64, device="cuda")
    with torch.no_grad():
        q.set_quant_state(True, True)
        q(batch)                                             # calibrate: one batch in estimate state
    q.learn_ranges()
    quantizers = {n: m.quantizer for n, m in _managers(q) if isinstance(m.quantizer, FPQuantizer)}
    ran, hooks = [], []
    for n, fq in quantizers.items():
        hooks.append(fq.register_forward_hook(lambda mod, a, y, n=n: ran.append(n)))
    captures, real = [], ops.quantize_backward

    def spy(x, g, mv, mb, n_bits, sb, *need, **kw):
        captures.append((x.detach().clone().contiguous(), g.detach().clone().contiguous(), mv.detach().clone(), float(mb),
                         n_bits, sb, mv.data_ptr()))
        return real(x, g, mv, mb, n_bits, sb, *need, **kw)
    monkeypatch.setattr(ops, "quantize_backward", spy)
    out = q(batch)
    (out * torch.randn_like(out)).sum().backward()
    monkeypatch.setattr(ops, "quantize_backward", real)
    for h in hooks:
        h.remove()
    # every quantizer the forward ran (a shared one may run more than once) has learned ranges, and every one of its calls
    # came back through the kernel route
    assert len(set(ran)) == N_CALLS[tag], (len(ran), len(set(ran)))
    by_ptr = {quantizers[n].maxval.data_ptr(): n for n in ran}
    assert len(by_ptr) == len(set(ran))
    assert len(captures) == len(ran) and {c[6] for c in captures} == set(by_ptr), "a quantizer's backward was not captured"
    for n in set(ran):
        p = quantizers[n].maxval
        assert isinstance(p, torch.nn.Parameter) and p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    n_pc = 0
    for x, g, mv, mb, n_bits, sb, ptr in captures:               # no capture skipped
        what = f"{tag} {by_ptr[ptr]} {tuple(x.shape)}"
        pc = mv.numel() > 1
        n_pc += pc
        gx, gmv, _ = real(x, g, mv, mb, n_bits, sb, True, True, False)
        y, cgx, cgmv, _ = _chain(x, g, mv, mb, n_bits, sb, monkeypatch)
        assert torch.equal(_bits(gx), _bits(cgx)), f"{what}: gx differs between the routes"
        sa, abs_a, _, _ = _host_sums(x, y, g, mv, sb, pc)
        got = gmv.cpu().numpy().astype(np.float64)
        assert np.isfinite(sa).all() and (np.abs(got - sa) <= BOUND * abs_a).all(), what
        # (the chain's own fp32 sums agree to their rounding: a loose cross-check that both routes mean the same quantity)
        np.testing.assert_allclose(cgmv.cpu().numpy().reshape(-1), sa, rtol=0, atol=1e-4 * float(abs_a.max()) + 1e-30, err_msg=what)
    assert n_pc > 0 and n_pc < len(captures)                      # per-channel weights and per-tensor activations
    print(f"\n{tag}: {len(captures)} quantizer backward calls replayed ({n_pc} per channel)")
