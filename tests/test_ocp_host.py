"""CPU-only checks of the hardware FP8 lane (csrc/fp8q_ocp.hip): the library exports its entry points and reports argument
errors before any launch, the Python wrappers refuse CPU tensors (there is no fallback), and OCPFP8Quantizer follows the
quantizer protocol without being one of the CLI's methods."""
import ctypes

import pytest
import torch

OCP = ("fp8q_ocp_encode_f32", "fp8q_ocp_encode_h16", "fp8q_ocp_decode_f32", "fp8q_ocp_decode_h16", "fp8q_ocp_quantize_f32",
       "fp8q_ocp_quantize_h16", "fp8q_ocp_scale_f32")
FMTS = (torch.float8_e4m3fn, torch.float8_e5m2)


def test_library_exports_every_ocp_symbol():
    import fp8q
    lib = ctypes.CDLL(fp8q.so_path())
    for n in OCP:
        assert hasattr(lib, n), n
        assert n in fp8q._lib.SIGNATURES, n
    assert {n for n in fp8q._lib.SIGNATURES if n.startswith("fp8q_ocp_")} == set(OCP)


def test_argument_errors_come_before_any_launch():
    import fp8q
    L = fp8q.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63             # never dereferenced: every call below is refused by the checks
    assert L.fp8q_ocp_encode_f32(None, p, 4, 4, p, 1, 0, 1e-8, None, None) == -1          # null x
    assert L.fp8q_ocp_encode_f32(p, p, 4, 4, p, 3, 0, 1e-8, None, None) == -1             # n_maxval not in {1, C}
    assert L.fp8q_ocp_encode_f32(p, p, 0, 4, p, 1, 0, 1e-8, None, None) == -1             # empty
    assert L.fp8q_ocp_encode_f32(p, p, 4, 4, p, 1, 2, 1e-8, None, None) == -2             # unknown format
    assert L.fp8q_ocp_encode_f32(p + 2, p, 4, 4, p, 1, 0, 1e-8, None, None) == -1         # misaligned fp32
    assert L.fp8q_ocp_encode_h16(p, p, 0, 4, 4, p, 1, 0, 1e-8, None, None) == -1          # x_type float32
    assert L.fp8q_ocp_encode_h16(p + 1, p, 1, 4, 4, p, 1, 0, 1e-8, None, None) == -1      # misaligned half
    assert L.fp8q_ocp_decode_f32(p, p, 4, 4, None, 1, 1, None) == -1                      # null scale
    assert L.fp8q_ocp_decode_h16(p, p, 0, 4, 4, p, 1, 1, None) == -1                      # y_type float32
    assert L.fp8q_ocp_quantize_f32(p, None, 4, 4, p, 1, 0, 1e-8, None) == -1
    assert L.fp8q_ocp_quantize_h16(p, p, 1, 2, 4, 4, p, 1, 0, 1e-8, None) == -1           # fp16 in, bf16 out
    assert L.fp8q_ocp_scale_f32(p, 0, 0, 1e-8, p, None) == -1
    assert L.fp8q_ocp_scale_f32(p, 4, 5, 1e-8, p, None) == -2


@pytest.mark.parametrize("fmt", FMTS)
def test_ops_raise_on_cpu_tensors(fmt):
    from fp8q import ops
    x = torch.randn(4, 4)
    mv = torch.ones(1)
    with pytest.raises(ops.Fp8qError):
        ops.ocp_encode(x, mv, fmt)
    with pytest.raises(ops.Fp8qError):
        ops.ocp_quantize(x, mv, fmt)
    with pytest.raises(ops.Fp8qError):
        ops.ocp_decode(torch.zeros(4, 4, dtype=torch.uint8).view(fmt), mv)
    with pytest.raises(ops.Fp8qError):
        ops.ocp_scale(mv, fmt)


def test_ops_refuse_other_formats():
    from fp8q import ops
    with pytest.raises(ops.Fp8qError):
        ops.ocp_quantize(torch.randn(4), torch.ones(1), torch.float16)
    if hasattr(torch, "float8_e4m3fnuz"):
        with pytest.raises(ops.Fp8qError):
            ops.ocp_encode(torch.randn(4), torch.ones(1), torch.float8_e4m3fnuz)


def test_quantizer_protocol_and_registry():
    from quantization.fp8 import QuantizerBase, QuantizerNotInitializedError
    from quantization.manager import QMethods, QuantizationManager
    from quantization.estimators import RangeEstimators
    from quantization.ocp import OCPFP8Quantizer
    assert issubclass(OCPFP8Quantizer, QuantizerBase)
    assert QMethods.list_names() == ["symmetric_uniform", "asymmetric_uniform", "fp_quantizer"]
    assert all(m.cls is not OCPFP8Quantizer for m in QMethods)
    q = OCPFP8Quantizer(per_channel=True, fmt=torch.float8_e5m2)
    assert q.n_bits == 8 and q.symmetric is True and q.is_initialized is False and q.fmax == 57344.0
    with pytest.raises(QuantizerNotInitializedError):
        q.range_maxval
    q.set_quant_range(torch.tensor([-2.0, 0.5, -1.0]), torch.tensor([1.0, 3.0, 1.0]))        # host tensors: torch ops only
    assert q.is_initialized and q.range_maxval.dtype == torch.float32
    assert q.range_maxval.tolist() == [2.0, 3.0, 1.0]
    assert "E5M2" in q.extra_repr() and "per_channel=True" in q.extra_repr()
    q.reset()
    assert not q.is_initialized
    with pytest.raises(ValueError):
        OCPFP8Quantizer(n_bits=4)
    with pytest.raises(ValueError):
        OCPFP8Quantizer(fmt=torch.float16)
    with pytest.raises(ValueError):
        OCPFP8Quantizer(per_channel=False).set_quant_range(torch.zeros(3), torch.ones(3))
    # the manager builds it like any other quantizer (the layers pass scale_domain along)
    mgr = QuantizationManager(qmethod=OCPFP8Quantizer, init=RangeEstimators.current_minmax.cls, per_channel=True,
                              qparams=dict(n_bits=8, scale_domain="linear", fmt=torch.float8_e4m3fn))
    assert isinstance(mgr.quantizer, OCPFP8Quantizer) and mgr.quantizer.per_channel
    with pytest.raises(QuantizerNotInitializedError):
        mgr.fix_ranges()


def test_quantizer_is_forward_only():
    from quantization.ocp import OCPFP8Quantizer
    q = OCPFP8Quantizer()
    q.set_quant_range(-1.0, 1.0)
    x = torch.randn(4, requires_grad=True)
    with pytest.raises(NotImplementedError):
        q(x)
    with pytest.raises(NotImplementedError):
        q.make_range_trainable()


def test_exporters_exist_next_to_the_others():
    from quantization.model import decode_ocp_weights, export_ocp_weights
    assert export_ocp_weights(torch.nn.Linear(2, 2)) == {}
    assert decode_ocp_weights({}) == {}
