"""INT8 ResNet-18 / MobileNetV2 with the fused INT epilogue (act_quant_kwargs=dict(fuse_epilogue=True)): the fused ops are
called at every site the FP8 model fuses, without a host synchronisation, and give the logits and the range buffers of their
two-launch compositions bit for bit; without the flag, or with the kernels or the fusion switched off, or under conditions
the kernel does not cover, the unfused chain runs as before."""
import copy
import io

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

FUSED = ("int_affine_act_quantize", "int_affine_act_range_quantize")


class _NoSync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


def _model(arch, kind, fuse=True, a_est="running_minmax"):
    """kind: 'sym' / 'asym' (INT8 uniform quantizers) or 'fp8' (the FP8 model whose fusion sites are the yardstick)"""
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    torch.manual_seed(0)
    kw = dict(weight_range_method=RangeEstimators.current_minmax.cls, act_range_method=RangeEstimators[a_est].cls, n_bits=8,
              n_bits_act=8, per_channel_weights=True)
    if kind == "fp8":
        kw.update(method=QMethods.fp_quantizer.cls, fp8_kwargs=dict(maxval=None, mantissa_bits=3, set_maxval=True))
    else:
        qm = QMethods.symmetric_uniform.cls if kind == "sym" else QMethods.asymmetric_uniform.cls
        kw.update(method=qm, act_method=qm)
        if fuse:
            kw.update(act_quant_kwargs=dict(fuse_epilogue=True))
    if arch == "r18":
        from models.resnet import resnet18
        from models.resnet_quantized import QuantizedResNet
        net = QuantizedResNet(resnet18(), input_size=(1, 3, 64, 64), **kw)
    else:
        from models.mobilenet_v2 import MobileNetV2
        from models.mobilenet_v2_quantized import QuantizedMobileNetV2
        net = QuantizedMobileNetV2(MobileNetV2(input_size=64), input_size=(1, 3, 64, 64), **kw)
    net = net.cuda().eval()
    net.quantized_weights()
    net.quantized_acts()
    return net


def _batches(seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(8, 3, 64, 64, device="cuda", generator=g) for _ in range(2)]


def _run(net, xs, guard=False):
    """two calibration batches, fixed ranges, one validation forward; returns the logits"""
    import contextlib
    nosync = _NoSync if guard else contextlib.nullcontext
    net.estimate_ranges()
    with torch.no_grad():
        with nosync():
            for x in xs:
                net(x)
        net.fix_ranges()
        with nosync():
            return net(xs[0])


def _count(monkeypatch, names):
    """wrap fp8q.ops.<name> with a call counter"""
    from fp8q import ops
    calls = dict.fromkeys(names, 0)
    for name in names:
        def wrapped(*a, _f=getattr(ops, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


@pytest.fixture(scope="module")
def fp8_sites():
    """affine_act_quantize calls of the FP8 model over the same two calibration batches and one validation forward"""
    from fp8q import ops
    out = {}
    for arch in ("r18", "mbv2"):
        n, orig = [0], ops.affine_act_quantize

        def wrapped(*a, **k):
            n[0] += 1
            return orig(*a, **k)
        ops.affine_act_quantize = wrapped
        try:
            _run(_model(arch, "fp8"), _batches())
        finally:
            ops.affine_act_quantize = orig
        out[arch] = n[0]
    return out


def _compose(monkeypatch):
    """the two fused ops replaced by their two-launch compositions"""
    from fp8q import ops

    def fixed(x, delta, zero_float, signed_flag, n_bits, symmetric, eps, bn_ab=None, residual=None, act=0, out=None):
        return ops.int_quantize(ops.affine_act(x, bn_ab, residual, act), delta, zero_float, signed_flag, n_bits, symmetric, eps,
                                out=out)

    def ranged(x, x_min, x_max, n_bits, symmetric, eps, delta=None, zero_float=None, signed_flag=None, bn_ab=None,
               residual=None, act=0, out=None):
        return ops.int_range_quantize(ops.affine_act(x, bn_ab, residual, act), x_min, x_max, n_bits, symmetric, eps, delta,
                                      zero_float, signed_flag, out=out)
    monkeypatch.setattr(ops, FUSED[0], fixed)
    monkeypatch.setattr(ops, FUSED[1], ranged)


@pytest.mark.parametrize("arch", ["r18", "mbv2"])
@pytest.mark.parametrize("kind", ["sym", "asym"])
def test_fused_int8_model(arch, kind, fp8_sites, monkeypatch):
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        xs = _batches()
        with monkeypatch.context() as mp:
            calls = _count(mp, FUSED)
            a = _model(arch, kind)
            ya = _run(a, xs, guard=True)              # calibration and validation without a host synchronisation
        # every site the FP8 model fuses: two estimating forwards (the range variant), one with fixed ranges
        assert sum(calls.values()) == fp8_sites[arch] > 0
        assert calls[FUSED[1]] == 2 * calls[FUSED[0]] > 0
        with monkeypatch.context() as mp:
            _compose(mp)
            b = _model(arch, kind)
            yb = _run(b, xs)
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
        sa, sb = a.state_dict(), b.state_dict()
        assert sa.keys() == sb.keys() and any(k.endswith("_delta") for k in sa)
        for k in sa:
            ta, tb = sa[k], sb[k]
            assert ta.dtype == tb.dtype and ta.shape == tb.shape, k
            assert torch.equal(ta.float().view(torch.int32), tb.float().view(torch.int32)), k
        # a calibrated model still copies and pickles
        with torch.no_grad():
            assert torch.equal(copy.deepcopy(a)(xs[0]).view(torch.int32), ya.view(torch.int32))
            buf = io.BytesIO()
            torch.save(a, buf)
            buf.seek(0)
            assert torch.equal(torch.load(buf, weights_only=False)(xs[0]).view(torch.int32), ya.view(torch.int32))
    finally:
        torch.backends.cudnn.deterministic = det


@pytest.mark.parametrize("how", ["no flag", "FP8Q_INT_KERNELS", "FP8Q_FUSE_EPILOGUE"])
def test_no_fused_op_without_the_flag_or_with_a_switch_off(how, monkeypatch):
    calls = _count(monkeypatch, FUSED)
    if how != "no flag":
        monkeypatch.setenv(how, "0")
    _run(_model("r18", "sym", fuse=how != "no flag"), _batches())
    assert sum(calls.values()) == 0


def _layer(qm, **kw):
    """conv + BN + ReLU as one quantized layer, activations quantized with `qm` built with fuse_epilogue=True"""
    from quantization.layers import BNQConv
    torch.manual_seed(1)
    args = dict(method=qm, act_method=qm, n_bits=8, n_bits_act=8, act_quant_kwargs=dict(fuse_epilogue=True))
    args.update(kw)
    layer = BNQConv(4, 8, 3, padding=1, activation=nn.ReLU(), **args).cuda().eval()
    layer.quantized_weights()
    layer.quantized_acts()
    return layer


@pytest.mark.parametrize("sym", [True, False])
def test_uncovered_conditions_fall_back(sym, monkeypatch):
    """line search, learned ranges, half input and per-channel activations keep the unfused chain: no fused op, no error"""
    from quantization.estimators import LineSearchEstimator
    from quantization.quantization_manager import QMethods, QuantizationManager
    qm = QMethods.symmetric_uniform.cls if sym else QMethods.asymmetric_uniform.cls
    x = torch.randn(2, 4, 6, 6, device="cuda")
    with torch.no_grad():
        probe = _layer(qm)
        with monkeypatch.context() as mp:
            seen = _count(mp, FUSED)
            probe(x)
            probe.fix_ranges()
            probe(x)
        assert seen[FUSED[1]] == 1 and seen[FUSED[0]] == 1          # (this layer does fuse when nothing is in the way)
    learned = _layer(qm)
    with torch.no_grad():
        learned(x)                                                  # (calibrated by the fused launch, then learned)
    learned.learn_ranges()
    calls = _count(monkeypatch, FUSED)
    with torch.no_grad():
        ls = _layer(qm, act_range_method=LineSearchEstimator, act_range_options=dict(num_candidates=50))
        assert ls(x).shape == (2, 8, 6, 6)
    y = learned(x)
    assert y.requires_grad
    y.sum().backward()
    assert learned.activation_quantizer.quantizer._delta.grad is not None
    with torch.no_grad():
        assert not learned(x).requires_grad
        keep = dict(keep_dtype=True)
        half = _layer(qm, act_quant_kwargs=dict(fuse_epilogue=True, **keep), weight_quant_kwargs=keep).half()
        assert half(x.half()).dtype == torch.float16
        mgr = QuantizationManager(qmethod=qm, per_channel=True, qparams=dict(n_bits=8, fuse_epilogue=True))
        assert not mgr.can_fuse(torch.randn(8, 4, 6, 6, device="cuda"))
        assert not probe.activation_quantizer.can_fuse(x.half())
        assert probe.activation_quantizer.can_fuse(x)
    assert sum(calls.values()) == 0
