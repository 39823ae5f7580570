"""Model level: a quantized CNN held in bfloat16 / float16 (keep_dtype=True) exports its weights as storage codes straight
from the half tensors (quantization.base_quantized_model export_fp8_weights / export_int_weights), and decoding them to the
model's dtype gives, bit for bit, the tensors the layers compute with.  float32 models export what they always did."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)


def _net():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1, bias=False), nn.BatchNorm2d(16), nn.ReLU(),
                        nn.Conv2d(16, 24, 3, stride=2, padding=1, bias=True), nn.ReLU6(),
                        nn.Conv2d(24, 24, 3, padding=1, groups=24, bias=False), nn.BatchNorm2d(24), nn.ReLU(),
                        nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(24, 10))
    return net.eval()


def _calibrated(dtype, **quant):
    from quantization.autoquant_utils import quantize_model
    from quantization.base_quantized_classes import QuantizedModule
    q = quantize_model(_net(), per_channel_weights=True, **quant).eval().cuda()
    if dtype != torch.float32:
        q = q.to(dtype)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in q.modules():
            if isinstance(m, QuantizedModule):
                m.quantized()
        q(torch.randn(8, 3, 16, 16, generator=g).cuda().to(dtype))
        for m in q.modules():
            if isinstance(m, QuantizedModule):
                m.fix_ranges()
    return q


def _fp8(dtype, keep=True):
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    return _calibrated(dtype, method=QMethods.fp_quantizer.cls, weight_range_method=RangeEstimators.current_minmax.cls,
                       act_range_method=RangeEstimators.allminmax.cls, n_bits=8,
                       fp8_kwargs=dict(maxval=None, mantissa_bits=3, set_maxval=True, keep_dtype=keep))


def _int(dtype, sym, n_bits, keep=True):
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    qm = QMethods.symmetric_uniform.cls if sym else QMethods.asymmetric_uniform.cls
    kw = dict(act_quant_kwargs=dict(keep_dtype=True), weight_quant_kwargs=dict(keep_dtype=True)) if keep else {}
    return _calibrated(dtype, method=qm, act_method=qm, weight_range_method=RangeEstimators.current_minmax.cls,
                       act_range_method=RangeEstimators.running_minmax.cls, n_bits=n_bits, n_bits_act=8, **kw)


def _layers(q):
    from quantization.hijacker import QuantizationHijacker
    return {n: m for n, m in q.named_modules() if isinstance(m, QuantizationHijacker)}


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


@pytest.mark.parametrize("dtype", DTYPES)
def test_export_fp8_weights_of_a_half_model(dtype):
    from quantization.base_quantized_model import export_fp8_weights, decode_fp8_weights
    q = _fp8(dtype)
    with torch.no_grad():
        layers = _layers(q)
        exported = export_fp8_weights(q)
        assert set(exported) == set(layers) and len(exported) == 4
        decoded = decode_fp8_weights(exported, dtype=dtype)
        for name, m in layers.items():
            assert m.weight.dtype == dtype
            assert exported[name]["codes"].dtype == torch.uint8 and exported[name]["codes"].shape == m.weight.shape
            assert exported[name]["maxval"].dtype == torch.float32
            want = m.get_params()[0]
            assert want.dtype == dtype and _same_bits(decoded[name], want), name


@pytest.mark.parametrize("sym,n_bits", [(True, 8), (False, 8), (True, 16)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_export_int_weights_of_a_half_model(dtype, sym, n_bits):
    from quantization.base_quantized_model import export_int_weights, decode_int_weights
    q = _int(dtype, sym, n_bits)
    with torch.no_grad():
        layers = _layers(q)
        exported = export_int_weights(q)
        assert set(exported) == set(layers) and len(exported) == 4
        decoded = decode_int_weights(exported, dtype=dtype)
        for name, m in layers.items():
            assert m.weight.dtype == dtype
            e = exported[name]
            assert e["codes"].dtype == (torch.uint8 if n_bits <= 8 else torch.int16) and e["codes"].shape == m.weight.shape
            assert e["n_bits"] == n_bits and e["symmetric"] == sym and e["delta"].dtype == torch.float32
            want = m.get_params()[0]
            assert want.dtype == dtype and _same_bits(decoded[name], want), name


def test_float32_models_export_what_they_did():
    """regression guard: the float32 route is the float32 entry points on the float32 weight, byte for byte"""
    from fp8q import ops
    from quantization.base_quantized_model import (export_fp8_weights, decode_fp8_weights, export_int_weights,
                                                   decode_int_weights)
    with torch.no_grad():
        q = _fp8(torch.float32, keep=False)
        exported = export_fp8_weights(q)
        decoded = decode_fp8_weights(exported)
        assert len(exported) == 4
        for name, m in _layers(q).items():
            wq = m.weight_quantizer.quantizer
            w = m.get_weight_bias()[0].detach().contiguous()
            assert w.dtype == torch.float32
            mv = wq.maxval.detach().float().reshape(-1)
            want = ops.encode(w, mv, float(wq.mantissa_bits), int(wq.n_bits), int(wq.sign_bits))
            assert torch.equal(exported[name]["codes"], want.cpu()), name
            assert decoded[name].dtype == torch.float32 and _same_bits(decoded[name], m.get_params()[0]), name
        for sym in (True, False):
            q = _int(torch.float32, sym, 8, keep=False)
            exported = export_int_weights(q)
            decoded = decode_int_weights(exported)
            assert len(exported) == 4
            for name, m in _layers(q).items():
                wq = m.weight_quantizer.quantizer
                w = m.get_weight_bias()[0].detach().contiguous()
                assert torch.equal(exported[name]["codes"], wq.encode(w).cpu()), name
                assert torch.equal(exported[name]["codes"], ops.int_encode(w, *wq._range_args()).cpu()), name
                assert decoded[name].dtype == torch.float32 and _same_bits(decoded[name], m.get_params()[0]), name
