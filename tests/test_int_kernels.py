"""Uniform (INT) quantizers on the HIP kernels (csrc/fp8q_int.hip): bit for bit the eager torch chain
(FP8Q_INT_KERNELS=0), the kernel path actually taken, and calibration / validation of INT8 models without a host
synchronisation.

Where torch's CUDA chain and its CPU chain differ, the CPU chain (which tests/test_int_golden.py pins to the reference)
decides: set_quant_range's `delta = (...) / int_max` divides by a Python number, which ATen's CUDA kernels evaluate as
a multiplication by the reciprocal, so on CUDA the eager ranges are off by an ulp for some inputs.  The range buffers
are therefore compared with the CPU chain, the quantize step with the CUDA chain on the same buffers."""
import copy
import io
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class _NoSync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


class _Eager:
    """FP8Q_INT_KERNELS=0 for the duration: the reference's torch op chain on the same device"""
    def __enter__(self):
        self.prev = os.environ.get("FP8Q_INT_KERNELS")
        os.environ["FP8Q_INT_KERNELS"] = "0"

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop("FP8Q_INT_KERNELS", None)
        else:
            os.environ["FP8Q_INT_KERNELS"] = self.prev
        return False


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_nan(a, b):
    """equal bits where not NaN, NaN at the same places (the sign of a NaN is not part of the contract)"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and _same(a.nan_to_num(0.0), b.nan_to_num(0.0))


def _quantizer(sym, n_bits, per_channel):
    from quantization.uniform import SymmetricUniformQuantizer, AsymmetricUniformQuantizer
    return (SymmetricUniformQuantizer if sym else AsymmetricUniformQuantizer)(n_bits=n_bits, per_channel=per_channel)


def _on_cuda_copy(q):
    """a quantizer with the same range buffers (copies), for the eager CUDA chain"""
    qb = copy.deepcopy(q)
    qb._delta = q._delta.clone()
    if q.symmetric:
        qb._signed = q._signed.clone()
    else:
        qb._zero_float = q._zero_float.clone()
    return qb


def _adversarial(shape, g):
    x = torch.randn(*shape, generator=g) * 3.0
    f = x.view(-1)
    n = f.numel()
    idx = torch.randperm(n, generator=g)
    k = max(n // 16, 1)
    f[idx[:k]] = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1e30, -1e30, float("inf"), float("-inf")]).repeat(k)[:k]
    return x


def _ties(x, q):
    """put exact rounding ties (k + 0.5) * delta of the quantizer's range into every 7th element"""
    d = q._delta.reshape(-1, *([1] * (x.dim() - 1))) if q._delta.dim() else q._delta
    k = torch.randint(-20, 20, x.shape, generator=torch.Generator().manual_seed(3)).float()
    t = ((k + 0.5) * d.cpu()).expand_as(x)
    m = torch.zeros(x.numel(), dtype=torch.bool)
    m[::7] = True
    return torch.where(m.view(x.shape), t, x)


CASES = [((4, 16, 14, 14), False), ((64, 3, 7, 7), True), ((1000, 512), True), ((7, 13, 3), True), ((5, 4099), True),
         ((1,), False), ((1, 5), True), ((3, 1, 1), True), ((33,), False), ((2, 70001), False), ((3000, 1), True)]


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("n_bits", [2, 4, 8, 16])
@pytest.mark.parametrize("shape,per_channel", CASES)
def test_kernel_equals_eager_chain(sym, n_bits, shape, per_channel):
    g = torch.Generator().manual_seed(hash((shape, n_bits)) % 1000)
    x = _adversarial(shape, g)
    C = shape[0] if per_channel else 1
    xmin = (-torch.rand(C, generator=g) * 4) if per_channel else -torch.rand((), generator=g) * 4
    xmax = (torch.rand(C, generator=g) * 4) if per_channel else torch.rand((), generator=g) * 4
    if per_channel and C > 2:
        xmin[1] = 0.0
        xmax[1] = 0.0                                # degenerate channel: xmin == xmax == 0
        xmin[2] = 0.25                               # positive minimum
    for xm_ in ((xmin, xmax), (xmin.abs(), xmax)):   # the second: non-negative ranges (symmetric: unsigned)
        qa, qc = _quantizer(sym, n_bits, per_channel), _quantizer(sym, n_bits, per_channel)
        qa.set_quant_range(xm_[0].cuda(), xm_[1].cuda())
        qc.set_quant_range(xm_[0], xm_[1])                      # the eager chain on the CPU
        assert _same(qa._delta, qc._delta)
        if sym:
            assert bool(qa._signed) == bool(qc._signed) and qa._signed.dtype == torch.bool and qa._signed.dim() == 0
        else:
            assert _same(qa._zero_float, qc._zero_float)
        qb = _on_cuda_copy(qa)
        xx = _ties(x, qc)
        ya = qa(xx.cuda())
        with _Eager():
            yb = qb(xx.cuda())
        assert _same(ya, yb), (shape, n_bits, sym)
        assert _same(ya, qc(xx)), (shape, n_bits, sym)
    # non-contiguous input
    xt = x.cuda().transpose(0, -1) if x.dim() > 1 else x.cuda()[::2]
    if not per_channel:
        with _Eager():
            yb = qb(xt)
        assert _same(qa(xt), yb)


def _one_float_off(n):
    """n floats of device memory that start one float behind a 16-byte boundary"""
    t = torch.empty(n + 1, device="cuda")[1:]
    assert t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("n_bits", [8, 16])
@pytest.mark.parametrize("shape,per_channel", CASES)
def test_views_off_a_16_byte_boundary_equal_the_aligned_call(sym, n_bits, shape, per_channel):
    """x, out=, or both one float off a 16-byte boundary -- the element-by-element (VEC = false) form of k_int_quant, with
    fixed ranges and range-setting -- against the aligned call, bit for bit."""
    from fp8q import ops
    g = torch.Generator().manual_seed(hash((shape, n_bits)) % 1000)
    x = _adversarial(shape, g)
    C = shape[0] if per_channel else 1
    xmin, xmax = (-torch.rand(C, generator=g) * 4).cuda(), (torch.rand(C, generator=g) * 4).cuda()
    delta, zf, sf = ops.int_set_range(xmin, xmax, n_bits, sym)
    xg = _ties(x, types.SimpleNamespace(_delta=delta)).cuda()
    assert xg.data_ptr() % 16 == 0
    xo = _one_float_off(xg.numel()).view(shape).copy_(xg)
    ya = ops.int_quantize(xg, delta, zf, sf, n_bits, sym)
    ra = ops.int_range_quantize(xg, xmin, xmax, n_bits, sym)
    assert ya.data_ptr() % 16 == 0 and ra[0].data_ptr() % 16 == 0
    for xi, off_out in ((xo, False), (xg, True), (xo, True)):
        out = _one_float_off(xg.numel()).view(shape) if off_out else None
        y = ops.int_quantize(xi, delta, zf, sf, n_bits, sym, out=out)
        assert (y is out or out is None) and _same(y, ya), (shape, n_bits, sym, off_out)
        out = _one_float_off(xg.numel()).view(shape) if off_out else None
        r = ops.int_range_quantize(xi, xmin, xmax, n_bits, sym, out=out)
        assert (r[0] is out or out is None) and _same(r[0], ra[0]), (shape, n_bits, sym, off_out)
        assert _same(r[1], ra[1]) and _same(r[1], delta)
        if sym:
            assert bool(r[3]) == bool(ra[3]) == bool(sf)
        else:
            assert _same(r[2], ra[2]) and _same(r[2], zf)


@pytest.mark.parametrize("sym", [True, False])
def test_nan_ranges_and_inputs(sym):
    nan = float("nan")
    q, qc = _quantizer(sym, 8, True), _quantizer(sym, 8, True)
    xmin = torch.tensor([-1.0, nan, -2.0, 0.0], device="cuda")
    xmax = torch.tensor([1.0, 1.0, nan, 3.0], device="cuda")
    q.set_quant_range(xmin, xmax)
    qc.set_quant_range(xmin.cpu(), xmax.cpu())
    assert _same_nan(q._delta, qc._delta)
    qe = _on_cuda_copy(q)
    x = torch.tensor([[0.3, nan, -5.0, 7.0], [1.0, 2.0, 3.0, 4.0], [nan, 1.0, -1.0, 0.0], [1.5, -0.2, 1e9, -1e9]],
                     device="cuda")
    with _Eager():
        ye = qe(x)
    y = q(x)
    assert torch.equal(torch.isnan(y), torch.isnan(ye)) and torch.equal(y.nan_to_num(123.0), ye.nan_to_num(123.0))
    if sym:
        assert not bool(q._signed)                   # a NaN minimum: NaN < 0 is false


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("per_channel", [False, True])
def test_bulk_tensor(sym, per_channel):
    torch.manual_seed(1)
    x = torch.randn(1 << 21, 3, 7, 7, device="cuda")
    q, qc = _quantizer(sym, 8, per_channel), _quantizer(sym, 8, per_channel)
    if per_channel:
        mn, mx = x.view(x.shape[0], -1).aminmax(dim=1)
    else:
        mn, mx = x.aminmax()
    q.set_quant_range(mn, mx)
    qc.set_quant_range(mn.cpu(), mx.cpu())
    assert _same(q._delta, qc._delta)
    qe = _on_cuda_copy(q)
    with _Eager():
        ye = qe(x)
    y = q(x)
    assert torch.equal(y.view(torch.int32), ye.view(torch.int32))


def test_the_kernel_path_is_taken(monkeypatch):
    q = _quantizer(True, 8, False)
    q.set_quant_range(torch.tensor(-1.0, device="cuda"), torch.tensor(2.0, device="cuda"))
    x = torch.randn(100, device="cuda")

    def boom(*a, **k):
        raise AssertionError("eager chain used")
    monkeypatch.setattr(torch, "round", boom)
    q(x)
    qa = _quantizer(False, 8, True)
    qa.set_quant_range(torch.full((4,), -1.0, device="cuda"), torch.full((4,), 2.0, device="cuda"))
    qa(torch.randn(4, 9, device="cuda"))
    monkeypatch.setenv("FP8Q_INT_KERNELS", "0")
    with pytest.raises(AssertionError, match="eager chain"):
        q(x)


def test_manager_estimating_paths_match_eager():
    from quantization.quantization_manager import QuantizationManager, QMethods
    from quantization.range_estimators import RangeEstimators
    torch.manual_seed(4)
    batches = [torch.randn(6, 5, 9, 9, device="cuda") * (i + 1) for i in range(3)]
    batches[1] = batches[1].abs()
    for qm in (QMethods.symmetric_uniform, QMethods.asymmetric_uniform):
        for est in ("current_minmax", "allminmax", "running_minmax"):
            for pc in (False, True):
                mk = lambda: QuantizationManager(qmethod=qm.cls, init=RangeEstimators[est].cls, per_channel=pc,
                                                 qparams=dict(n_bits=8))
                a = mk()
                for x in batches:
                    ya = a(x)
                    c = qm.cls(n_bits=8, per_channel=pc)            # the eager chain on the CPU, same ranges
                    c.set_quant_range(a.range_estimator.current_xmin.cpu(), a.range_estimator.current_xmax.cpu())
                    assert _same(ya, c(x.cpu())), (qm, est, pc)
                    assert _same(a.quantizer._delta.reshape(-1), c._delta.reshape(-1))
                a.fix_ranges()
                assert _same(a(batches[0]), c(batches[0].cpu()))


def _int_model(arch, sym, w_est="current_minmax", a_est="running_minmax", method=None):
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    torch.manual_seed(0)
    qm = QMethods.symmetric_uniform.cls if sym else QMethods.asymmetric_uniform.cls
    kw = dict(method=method or qm, act_method=qm, weight_range_method=RangeEstimators[w_est].cls,
              act_range_method=RangeEstimators[a_est].cls, n_bits=8, n_bits_act=8, per_channel_weights=True)
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


def _calibrate(net, xs, guard):
    net.estimate_ranges()
    with torch.no_grad():
        if guard:
            with _NoSync():
                for x in xs:
                    net(x)
        else:
            for x in xs:
                net(x)
    net.fix_ranges()


@pytest.mark.parametrize("arch", ["r18", "mbv2"])
@pytest.mark.parametrize("sym", [True, False])
def test_int8_model_calibration_and_validation_are_sync_free(arch, sym):
    torch.manual_seed(7)
    xs = [torch.randn(8, 3, 64, 64, device="cuda") for _ in range(2)]
    net = _int_model(arch, sym)
    _calibrate(net, xs, guard=True)
    with torch.no_grad(), _NoSync():
        net(xs[0])
        net(xs[1])


@pytest.mark.parametrize("arch", ["r18", "mbv2"])
@pytest.mark.parametrize("sym", [True, False])
def test_int8_model_logits_match_the_eager_chain(arch, sym):
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(8)
        xs = [torch.randn(8, 3, 64, 64, device="cuda") for _ in range(2)]
        a = _int_model(arch, sym)
        _calibrate(a, xs, guard=False)
        with torch.no_grad():
            ya = a(xs[0])
        with _Eager():
            # (calibrating with the eager chain would give ranges off by an ulp: see the module docstring)
            b = _int_model(arch, sym)
            _calibrate(b, xs[:1], guard=False)
            b.load_state_dict(a.state_dict())
            with torch.no_grad():
                yb = b(xs[0])
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    finally:
        torch.backends.cudnn.deterministic = det


def test_copy_save_load_and_the_weight_cache():
    # (deterministic convolutions, as in the test above: four forwards of equal networks are compared bit for bit, and inside
    # a full run of the suite the library's convolutions did not always repeat their own bits -- one logit a grid step off)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(9)
        xs = [torch.randn(4, 3, 64, 64, device="cuda") for _ in range(2)]
        net = _int_model("r18", True)
        _calibrate(net, xs, guard=False)
        with torch.no_grad():
            y0 = net(xs[0])
            y1 = copy.deepcopy(net)(xs[0])
            buf = io.BytesIO()
            torch.save(net, buf)
            buf.seek(0)
            y2 = torch.load(buf, weights_only=False)(xs[0])
            other = _int_model("r18", True)
            _calibrate(other, [xs[1]], guard=False)
            other.load_state_dict(net.state_dict())
            y3 = other(xs[0])
    finally:
        torch.backends.cudnn.deterministic = det
    for y in (y1, y2, y3):
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32))
    # a range change invalidates the cached quantized weight
    from quantization.layers import QuantizationHijacker
    layer = next(m for m in net.modules() if isinstance(m, QuantizationHijacker) and m._qw)
    q = layer.weight_quantizer.quantizer
    w = layer.get_weight_bias()[0]
    with torch.no_grad():
        c0 = layer._quantized_weight(w)
        assert layer._quantized_weight(w) is c0
        q.set_quant_range(q.x_min_fp32 * 2, q.x_max_fp32 * 2)
        c1 = layer._quantized_weight(w)
    assert c1 is not c0 and not torch.equal(c1, c0)
