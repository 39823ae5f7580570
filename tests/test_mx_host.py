"""CPU-only checks of the microscaling lane (csrc/fp8q_mx.hip): the library exports its six entry points and reports argument
errors before any launch, the Python wrappers refuse CPU tensors and foreign formats (there is no fallback), and MXQuantizer
follows the quantizer protocol without being one of the CLI's methods or ever giving its manager's estimator work."""
import ctypes

import pytest
import torch

MX = ("fp8q_mx_encode_f32", "fp8q_mx_encode_h16", "fp8q_mx_decode_f32", "fp8q_mx_decode_h16", "fp8q_mx_quantize_f32",
      "fp8q_mx_quantize_h16")
FMTS = (torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2)
E4M3FN, E5M2, E2M1 = 0, 1, 2
FLOOR, CEIL = 0, 1
F16, BF16 = 1, 2


def test_library_exports_exactly_the_six_mx_symbols():
    import fp8q
    lib = ctypes.CDLL(fp8q.so_path())
    for n in MX:
        assert hasattr(lib, n), n
        assert n in fp8q._lib.SIGNATURES, n
    assert {n for n in fp8q._lib.SIGNATURES if n.startswith("fp8q_mx_")} == set(MX)
    assert fp8q.lib().fp8q_version() == 601           # the entries are additive


def test_argument_errors_come_before_any_launch():
    import fp8q
    L = fp8q.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63             # never dereferenced: every call below is refused by the checks
    enc, ench = L.fp8q_mx_encode_f32, L.fp8q_mx_encode_h16
    dec, dech = L.fp8q_mx_decode_f32, L.fp8q_mx_decode_h16
    qnt, qnth = L.fp8q_mx_quantize_f32, L.fp8q_mx_quantize_h16
    # null pointers
    assert enc(None, p, p, 4, 32, E4M3FN, FLOOR, None) == -1
    assert enc(p, None, p, 4, 32, E4M3FN, FLOOR, None) == -1
    assert enc(p, p, None, 4, 32, E4M3FN, FLOOR, None) == -1
    assert dec(None, p, p, 4, 32, E5M2, None) == -1
    assert dec(p, None, p, 4, 32, E5M2, None) == -1
    assert dec(p, p, None, 4, 32, E5M2, None) == -1
    assert qnt(None, p, 4, 32, E2M1, CEIL, None) == -1
    assert qnt(p, None, 4, 32, E2M1, CEIL, None) == -1
    # empty tensors
    assert enc(p, p, p, 0, 32, E4M3FN, FLOOR, None) == -1
    assert enc(p, p, p, 4, 0, E4M3FN, FLOOR, None) == -1
    assert dec(p, p, p, 4, -1, E4M3FN, None) == -1
    assert qnt(p, p, 0, 0, E4M3FN, FLOOR, None) == -1
    # a misaligned value pointer (codes and scale bytes may lie anywhere)
    assert enc(p + 2, p, p, 4, 32, E4M3FN, FLOOR, None) == -1
    assert ench(p + 1, p, p, F16, 4, 32, E4M3FN, FLOOR, None) == -1
    assert dec(p, p, p + 2, 4, 32, E4M3FN, None) == -1
    assert dech(p, p, p + 1, BF16, 4, 32, E4M3FN, None) == -1
    assert qnt(p, p + 1, 4, 32, E4M3FN, FLOOR, None) == -1
    assert qnth(p + 1, p, F16, F16, 4, 32, E4M3FN, FLOOR, None) == -1
    # an odd K with E2M1
    assert enc(p, p, p, 4, 33, E2M1, FLOOR, None) == -1
    assert dec(p, p, p, 4, 1, E2M1, None) == -1
    assert qnt(p, p, 4, 31, E2M1, FLOOR, None) == -1
    # an unknown format, an unknown rounding
    assert enc(p, p, p, 4, 32, 3, FLOOR, None) == -2
    assert dec(p, p, p, 4, 32, -1, None) == -2
    assert qnth(p, p, BF16, BF16, 4, 32, 7, FLOOR, None) == -2
    assert enc(p, p, p, 4, 32, E4M3FN, 2, None) == -1
    assert qnt(p, p, 4, 32, E4M3FN, -1, None) == -1
    # types: a half entry takes half types, quantize's y_type is float32 or x_type
    assert ench(p, p, p, 0, 4, 32, E4M3FN, FLOOR, None) == -1
    assert dech(p, p, p, 0, 4, 32, E4M3FN, None) == -1
    assert dech(p, p, p, 3, 4, 32, E4M3FN, None) == -1
    assert qnth(p, p, 0, 0, 4, 32, E4M3FN, FLOOR, None) == -1
    assert qnth(p, p, F16, BF16, 4, 32, E4M3FN, FLOOR, None) == -1
    assert qnth(p, p, BF16, F16, 4, 32, E4M3FN, FLOOR, None) == -1


@pytest.mark.parametrize("fmt", FMTS)
def test_ops_raise_on_cpu_tensors(fmt):
    from fp8q import ops
    x = torch.randn(4, 64)
    with pytest.raises(ops.Fp8qError):
        ops.mx_encode(x, fmt)
    with pytest.raises(ops.Fp8qError):
        ops.mx_quantize(x, fmt, rounding="ceil")
    kc = 32 if fmt == torch.float4_e2m1fn_x2 else 64
    codes = torch.zeros(4, kc, dtype=torch.uint8)
    scales = torch.full((4, 2), 127, dtype=torch.uint8)
    with pytest.raises(ops.Fp8qError):
        ops.mx_decode(codes.view(fmt), scales.view(torch.float8_e8m0fnu))
    with pytest.raises(ops.Fp8qError):
        ops.mx_decode(codes, scales, fmt=fmt)


def test_ops_refuse_other_formats_and_roundings():
    from fp8q import ops
    x = torch.randn(4, 64)
    for fmt in (torch.float16, torch.uint8, torch.float8_e8m0fnu, getattr(torch, "float8_e4m3fnuz", torch.int8)):
        with pytest.raises(ops.Fp8qError, match="fmt must be"):
            ops.mx_encode(x, fmt)
        with pytest.raises(ops.Fp8qError, match="fmt must be"):
            ops.mx_quantize(x, fmt)
    with pytest.raises(ops.Fp8qError, match="rounding"):
        ops.mx_encode(x, torch.float8_e4m3fn, rounding="nearest")
    with pytest.raises(ops.Fp8qError, match="rounding"):
        ops.mx_quantize(x, torch.float8_e4m3fn, rounding=None)
    with pytest.raises(ops.Fp8qError):                      # a half decode target exists, an integer one does not
        ops.mx_decode(torch.zeros(4, 64, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8), fmt=torch.float8_e5m2,
                      out_dtype=torch.int32)


def test_quantizer_protocol_and_registry():
    from quantization.fp8 import QuantizerBase
    from quantization.manager import QMethods
    from quantization.mx import MXQuantizer
    assert issubclass(MXQuantizer, QuantizerBase) and MXQuantizer.range_free is True
    assert QMethods.list_names() == ["symmetric_uniform", "asymmetric_uniform", "fp_quantizer"]
    assert all(m.cls is not MXQuantizer for m in QMethods)
    q = MXQuantizer()
    assert q.n_bits == 8 and q.fmt == torch.float8_e4m3fn and q.rounding == "floor" and not q.keep_dtype and not q.flatten_rows
    assert q.is_initialized is True and q.symmetric is True
    q.set_quant_range(torch.tensor(-1.0), torch.tensor(1.0))          # no-ops: there is no range
    q.reset()
    q.fix_ranges()
    assert q.is_initialized is True
    q4 = MXQuantizer(fmt=torch.float4_e2m1fn_x2, rounding="ceil", flatten_rows=True, per_channel=True, scale_domain="linear")
    assert q4.n_bits == 4 and "E2M1" in q4.extra_repr() and "ceil" in q4.extra_repr()
    assert MXQuantizer(n_bits=4, fmt=torch.float4_e2m1fn_x2).n_bits == 4
    with pytest.raises(ValueError):
        MXQuantizer(n_bits=8, fmt=torch.float4_e2m1fn_x2)
    with pytest.raises(ValueError):
        MXQuantizer(n_bits=4)
    with pytest.raises(ValueError):
        MXQuantizer(fmt=torch.float16)
    with pytest.raises(ValueError):
        MXQuantizer(rounding="up")
    # flatten_rows: [shape[0], -1] for more than two dimensions, the tensor itself otherwise
    w = torch.zeros(8, 3, 3, 3)
    assert tuple(q4._rows(w).shape) == (8, 27) and q4._rows(w[0, 0]).shape == (3, 3) and q._rows(w).shape == w.shape


def test_quantizer_is_forward_only():
    from quantization.mx import MXQuantizer
    q = MXQuantizer()
    with pytest.raises(NotImplementedError):
        q(torch.randn(4, 32, requires_grad=True))
    with pytest.raises(NotImplementedError):
        q.make_range_trainable()


def test_manager_never_gives_the_estimator_work():
    """in every state a range_free quantizer is called directly: the estimator object the manager builds is never called (a
    CPU tensor gets as far as the op's refusal, which is behind the point where an estimator would have run)"""
    from fp8q import ops
    from quantization.estimators import RangeEstimators
    from quantization.manager import QuantizationManager
    from quantization.mx import MXQuantizer
    mgr = QuantizationManager(qmethod=MXQuantizer, init=RangeEstimators.current_minmax.cls, per_channel=True,
                              qparams=dict(n_bits=8, scale_domain="linear", fmt=torch.float8_e5m2))
    assert isinstance(mgr.quantizer, MXQuantizer)
    calls = []
    mgr.range_estimator.register_forward_pre_hook(lambda m, a: calls.append(a))
    seen = []
    mgr.quantizer.register_forward_pre_hook(lambda m, a: seen.append(a[0].dtype))
    for enter in (mgr.estimate_ranges, mgr.estimate_ranges_train, mgr.fix_ranges):      # fix_ranges: always initialized
        enter()
        for x in (torch.randn(4, 32), torch.randn(4, 32).bfloat16()):
            with pytest.raises(ops.Fp8qError):
                mgr(x)
    assert calls == []
    assert seen == [torch.float32, torch.bfloat16] * 3           # half tensors reach the quantizer as they are
    mgr.reset_ranges()
    assert mgr.quantizer.is_initialized


def test_exporters_exist_next_to_the_others():
    from quantization.model import decode_mx_weights, export_mx_weights
    assert export_mx_weights(torch.nn.Linear(2, 2)) == {}
    assert decode_mx_weights({}) == {}
