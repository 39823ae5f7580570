"""The INT quantizers' backward where the models use it: one forward / backward of a quantized ResNet-18 with learned ranges
(symmetric per-channel weights, asymmetric per-tensor activations), once through the kernel route and once through the torch
chain (FP8Q_GRAD_KERNELS=0), on the same model, batch and upstream gradient.

  logits                 bit-identical (the forward kernel is the chain's arithmetic);
  range parameters       |kernel .grad - chain .grad| <= K_SUM * sum |term| per row, the bound of test_int_grad_golden.py, the
                         terms evaluated from the quantizer's own captured input and upstream gradient (summed over its calls);
                         a quantizer that ran once is also held to the kernel's own bound against the float64 host sum
                         (2^-22 * sum |term|, test_int_grad_kernels.py);
  weights                within 1e-5 * max |grad| of the chain's;
  and ops.int_quantize_backward ran for every INT quantizer of the model.
"""
import numpy as np
import pytest
import torch

from test_int_grad_golden import K_SUM, _contract
from test_models import _managers, _warm_bn

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -22


def _build():
    from models.resnet import resnet18
    from models.resnet_quantized import QuantizedResNet
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    torch.manual_seed(0)
    kw = dict(method=QMethods.symmetric_uniform.cls, act_method=QMethods.asymmetric_uniform.cls,
              weight_range_method=RangeEstimators.current_minmax.cls, act_range_method=RangeEstimators.allminmax.cls,
              n_bits=8, n_bits_act=8, per_channel_weights=True)
    return QuantizedResNet(_warm_bn(resnet18(pretrained=False)), input_size=(1, 3, 32, 32), **kw).eval()


def _step(q, batch, up):
    for p in q.parameters():
        p.grad = None
    out = q(batch)
    (out * up).sum().backward()
    return out.detach().clone(), {n: p.grad.detach().clone() for n, p in q.named_parameters() if p.grad is not None}


def test_resnet18_learned_int_ranges_kernel_route_against_chain(monkeypatch):
    from fp8q import ops
    from quantization.uniform import AsymmetricUniformQuantizer
    q = _build().cuda()
    torch.manual_seed(5)
    batch = torch.randn(2, 3, 32, 32, device="cuda")
    with torch.no_grad():
        q.set_quant_state(True, True)
        q(batch)                                             # calibrate: one batch in estimate state
    q.learn_ranges()
    quantizers = {n: m.quantizer for n, m in _managers(q) if isinstance(m.quantizer, AsymmetricUniformQuantizer)}
    ran, hooks = [], []
    for n, uq in quantizers.items():
        hooks.append(uq.register_forward_hook(lambda mod, a, y, n=n: ran.append(n)))
    captures, real = [], ops.int_quantize_backward

    def spy(x, g, delta, zf, flag, n_bits, symmetric, eps, *need, **kw):
        captures.append((x.detach().cpu().numpy(), g.detach().cpu().numpy(), delta.detach().cpu().numpy().reshape(-1),
                         None if zf is None else zf.detach().cpu().numpy().reshape(-1),
                         None if flag is None else bool(flag.item()), n_bits, symmetric, delta.data_ptr()))
        assert abs(eps - 1e-8) < 1e-12 and (need + (0,))[3] == 0 and not kw
        return real(x, g, delta, zf, flag, n_bits, symmetric, eps, *need, **kw)
    monkeypatch.setattr(ops, "int_quantize_backward", spy)
    torch.manual_seed(6)
    up = torch.randn(2, 1000, device="cuda")
    logits_k, grads_k = _step(q, batch, up)
    monkeypatch.setattr(ops, "int_quantize_backward", real)
    for h in hooks:
        h.remove()
    n_kernel = len(captures)
    monkeypatch.setenv("FP8Q_GRAD_KERNELS", "0")
    monkeypatch.setattr(ops, "int_quantize_backward", lambda *a, **k: pytest.fail("the chain route called the kernel"))
    logits_c, grads_c = _step(q, batch, up)

    assert torch.equal(logits_k.view(torch.int32), logits_c.view(torch.int32)), "the logits differ between the routes"
    # every INT quantizer the forward ran came back through the new op
    assert ran and set(ran) <= set(quantizers)
    by_ptr = {quantizers[n]._delta.data_ptr(): n for n in set(ran)}
    assert len(by_ptr) == len(set(ran))
    assert n_kernel == len(ran) and {c[7] for c in captures} == set(by_ptr), "a quantizer's backward did not take the kernel route"
    assert set(grads_k) == set(grads_c)

    # per range parameter: the sums of magnitudes of its calls
    mags, host, calls = {}, {}, {}
    for x, g, delta, zf, flag, n_bits, symmetric, ptr in captures:
        c = dict(kind="sym" if symmetric else "asym", signed=bool(flag), n_bits=n_bits)
        _, sa, abs_a, sb, abs_b = _contract(x, g, delta, zf, c)
        for key, s, mag in ((("d", ptr), sa, abs_a),) + (() if symmetric else ((("z", ptr), sb, abs_b),)):
            mags[key] = mags.get(key, 0.0) + mag
            host[key] = host.get(key, 0.0) + s
            calls[key] = calls.get(key, 0) + 1
    n_pc = n_checked = 0
    for n, uq in quantizers.items():
        if n not in ran:
            continue
        for tag, p in (("d", uq._delta),) + (() if uq.symmetric else (("z", uq._zero_float),)):
            assert isinstance(p, torch.nn.Parameter) and p.grad is not None, (n, tag)
            name = [pn for pn, pp in q.named_parameters() if pp is p][0]
            gk, gc = (grads[name].cpu().numpy().astype(np.float64).reshape(-1) for grads in (grads_k, grads_c))
            assert grads_k[name].shape == p.shape
            key = (tag, uq._delta.data_ptr())
            assert np.isfinite(gk).all() and np.isfinite(gc).all(), (n, tag)
            err = np.abs(gk - gc)
            print(f"{n} {tag}: kernel vs chain {float((err / np.maximum(mags[key], 1e-300)).max()):.3e} of sum |term| (bound {K_SUM:.1e})")
            assert (err <= K_SUM * mags[key]).all(), f"{n} {tag}: the routes differ by {(err / np.maximum(mags[key], 1e-300)).max():.3e} of sum |term|"
            if calls[key] == 1:
                assert (np.abs(gk - host[key]) <= BOUND * mags[key]).all(), f"{n} {tag}: kernel off its own host sum"
            n_pc += p.numel() > 1
            n_checked += 1
    assert n_checked >= len(set(ran)) and n_pc > 0 and n_pc < n_checked     # per-channel weights and per-tensor activations

    range_names = {pn for pn, pp in q.named_parameters() for uq in quantizers.values()
                   if pp is uq._delta or pp is getattr(uq, "_zero_float", None)}
    n_w = 0
    for name in grads_k:
        if name in range_names:
            continue
        gk, gc = grads_k[name], grads_c[name]
        tol = 1e-5 * float(gc.abs().max())
        err = float((gk - gc).abs().max())
        assert err <= tol, f"{name}: weight gradient differs by {err:.3e} (max |grad| {float(gc.abs().max()):.3e})"
        n_w += 1
    assert n_w > 20
    print(f"\nresnet18: {n_kernel} INT quantizer backward calls on the kernel route, {n_checked} range parameters, {n_w} other parameters compared")
