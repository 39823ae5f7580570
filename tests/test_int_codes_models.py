"""Model level: the weights of an INT8-calibrated ResNet-18 as integer codes (quantization.base_quantized_model
export_int_weights / decode_int_weights) -- one entry per layer with quantized weights, decoding to exactly the tensors the
layers compute with -- and the FP8 and INT exports each leaving the other lane's models alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _int_model(arch, sym, w_est="current_minmax", a_est="running_minmax", method=None):
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    torch.manual_seed(0)
    qm = QMethods.symmetric_uniform.cls if sym else QMethods.asymmetric_uniform.cls
    kw = dict(method=method or qm, act_method=qm, weight_range_method=RangeEstimators[w_est].cls,
              act_range_method=RangeEstimators[a_est].cls, n_bits=8, n_bits_act=8, per_channel_weights=True)
    assert arch == "r18"
    from models.resnet import resnet18
    from models.resnet_quantized import QuantizedResNet
    net = QuantizedResNet(resnet18(), input_size=(1, 3, 64, 64), **kw)
    net = net.cuda().eval()
    net.quantized_weights()
    net.quantized_acts()
    return net


def _calibrated(sym, method=None):
    torch.manual_seed(7)
    xs = [torch.randn(8, 3, 64, 64, device="cuda") for _ in range(2)]
    net = _int_model("r18", sym, method=method)
    net.estimate_ranges()
    with torch.no_grad():
        for x in xs:
            net(x)
    net.fix_ranges()
    return net


@pytest.mark.parametrize("sym", [True, False])
def test_export_int_weights_of_resnet18(sym):
    from quantization.base_quantized_model import export_fp8_weights, export_int_weights, decode_int_weights
    from quantization.hijacker import QuantizationHijacker
    net = _calibrated(sym)
    layers = {n: m for n, m in net.named_modules() if isinstance(m, QuantizationHijacker) and m._qw}
    assert len(layers) == 21                                 # 20 convolutions and the classifier
    with torch.no_grad():
        exported = export_int_weights(net)
        decoded = decode_int_weights(exported, "cuda")
        assert set(exported) == set(layers) and set(decoded) == set(layers)
        for name, m in layers.items():
            e = exported[name]
            q = m.weight_quantizer.quantizer
            w = m.get_weight_bias()[0]
            assert e["codes"].dtype == torch.uint8 and e["codes"].shape == w.shape and not e["codes"].is_cuda
            assert e["n_bits"] == 8 and e["symmetric"] == sym and e["eps"] == q.eps
            assert e["delta"].shape == (w.shape[0],) and not e["delta"].is_cuda
            if sym:
                assert e["zero_float"] is None and e["signed"].dtype == torch.bool and not e["signed"].is_cuda
                signed = bool(e["signed"])
                assert signed == bool(q._signed)
            else:
                assert e["signed"] is None and e["zero_float"].shape == (w.shape[0],) and not e["zero_float"].is_cuda
                signed = False
            ints = e["codes"].view(torch.int8).int() if signed else e["codes"].int()
            assert int(ints.min()) >= int(q.int_min) and int(ints.max()) <= int(q.int_max)
            assert ints.unique().numel() > 16                # the codes use the grid
            cached = m._quantized_weight(w)                  # what the layer computes with
            assert decoded[name].dtype == torch.float32 and decoded[name].shape == cached.shape
            assert torch.equal(decoded[name].view(torch.int32), cached.contiguous().view(torch.int32)), name
        assert export_fp8_weights(net) == {}


def test_an_fp8_model_exports_nothing_as_int():
    from quantization.base_quantized_model import export_fp8_weights, export_int_weights
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    from models.resnet import resnet18
    from models.resnet_quantized import QuantizedResNet
    torch.manual_seed(0)
    net = QuantizedResNet(resnet18(), input_size=(1, 3, 64, 64), method=QMethods.fp_quantizer.cls,
                          weight_range_method=RangeEstimators.current_minmax.cls,
                          act_range_method=RangeEstimators.allminmax.cls, n_bits=8, per_channel_weights=True,
                          fp8_kwargs=dict(maxval=None, mantissa_bits=3, set_maxval=True)).cuda().eval()
    net.quantized_weights()
    net.quantized_acts()
    net.estimate_ranges()
    with torch.no_grad():
        net(torch.randn(8, 3, 64, 64, device="cuda"))
        net.fix_ranges()
        assert export_int_weights(net) == {}
        assert len(export_fp8_weights(net)) == 21
