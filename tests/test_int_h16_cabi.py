"""CPU-only checks of the uniform (INT) entry points for float16 / bfloat16 tensors (csrc/fp8q_inth16.hip): the header
declares them, the library exports them, fp8q._lib binds them, and every argument error is reported before any launch, so it
is exercised without a GPU; the ops wrappers and the quantizers take the new options."""
import os
import re

import pytest

F32, F16, BF16 = 0, 1, 2
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
P = 4096                                     # a non-null, aligned pointer value that is never dereferenced (no launch)
ENTRIES = ("fp8q_int_quantize_h16", "fp8q_int_range_quantize_h16", "fp8q_int_minmax_quantize_h16")


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "fp8q.h")).read()


def test_header_declares_library_exports_lib_binds():
    import ctypes
    import fp8q
    from fp8q import _lib
    hdr = _header()
    raw = ctypes.CDLL(_lib.so_path())
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(const void \*x, void \*y, int x_type, int y_type, int64_t C, int64_t inner,", hdr,
                         re.M), name
        assert getattr(raw, name) is not None                                # exported (AttributeError otherwise)
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args[:6] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_int64, ctypes.c_int64]
        assert getattr(fp8q.lib(), name).argtypes == args
    assert len(_lib.SIGNATURES["fp8q_int_quantize_h16"][1]) == len(_lib.SIGNATURES["fp8q_int_quantize_f32"][1]) + 2
    assert len(_lib.SIGNATURES["fp8q_int_range_quantize_h16"][1]) == len(_lib.SIGNATURES["fp8q_int_range_quantize_f32"][1]) + 2
    assert len(_lib.SIGNATURES["fp8q_int_minmax_quantize_h16"][1]) == len(_lib.SIGNATURES["fp8q_int_minmax_quantize_f32"][1]) + 2
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr)
    assert fp8q.lib().fp8q_version() == 601


def test_int_quantize_h16_argument_validation_without_gpu():
    import fp8q
    q = fp8q.lib().fp8q_int_quantize_h16
    # (x, y, x_type, y_type, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps, stream)
    for xt in (F16, BF16):
        for yt in (F32, xt):
            assert q(None, P, xt, yt, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL      # null x
            assert q(P, None, xt, yt, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL      # null y
            assert q(P, P, xt, yt, 4, 8, None, P, 1, None, 8, 0, 1e-8, None) == EINVAL      # null delta
            assert q(P, P, xt, yt, 4, 8, P, None, 1, None, 8, 0, 1e-8, None) == EINVAL      # asymmetric without zero_float
            assert q(P, P, xt, yt, 4, 8, P, None, 1, None, 8, 1, 1e-8, None) == EINVAL      # symmetric without the sign
            assert q(P, P, xt, yt, 4, 8, P, P, 3, None, 8, 0, 1e-8, None) == EINVAL         # n_delta not in {1, C}
            assert q(P, P, xt, yt, 4, 8, P, P, 0, None, 8, 0, 1e-8, None) == EINVAL
            assert q(P, P, xt, yt, 0, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL         # empty
            assert q(P, P, xt, yt, 4, 0, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
            assert q(P, P, xt, yt, 4, -1, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
            assert q(P + 1, P, xt, yt, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL     # odd address of a 2-byte element
            # the size limits of int_check_x: a per-channel row beyond 2^31 - 1 elements, C * inner beyond int64, more
            # chunks than a grid holds
            assert q(P, P, xt, yt, 2, 1 << 31, P, P, 2, None, 8, 0, 1e-8, None) == EINVAL
            assert q(P, P, xt, yt, 1 << 40, 1 << 40, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
            assert q(P, P, xt, yt, 1, 1 << 45, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
            for nb in (1, 0, 17, 32):
                assert q(P, P, xt, yt, 4, 8, P, P, 4, None, nb, 0, 1e-8, None) == EUNSUPPORTED   # n_bits outside [2, 16]
                assert q(P, P, xt, yt, 4, 8, P, None, 1, P, nb, 1, 1e-8, None) == EUNSUPPORTED
        assert q(P, P + 2, xt, F32, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL        # fp32 output at a 2-byte phase
        assert q(P, P + 1, xt, xt, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
        assert q(P, P, xt, 3 - xt, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL         # y_type: the OTHER half type
        assert q(P, P, xt, 7, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
    for bad in (F32, 3, -1):                                                                # x_type is not a half type
        assert q(P, P, bad, F32, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL


def test_int_range_quantize_h16_argument_validation_without_gpu():
    import fp8q
    r = fp8q.lib().fp8q_int_range_quantize_h16
    # (x, y, x_type, y_type, C, inner, x_min, x_max, n_range, delta, zero_float, signed_flag, n_bits, symmetric, eps, stream)
    for xt in (F16, BF16):
        for yt in (F32, xt):
            assert r(None, P, xt, yt, 4, 8, P, P, 4, P, P, None, 8, 0, 1e-8, None) == EINVAL
            assert r(P, None, xt, yt, 4, 8, P, P, 4, P, P, None, 8, 0, 1e-8, None) == EINVAL
            assert r(P, P, xt, yt, 4, 8, None, P, 4, P, P, None, 8, 0, 1e-8, None) == EINVAL     # null x_min
            assert r(P, P, xt, yt, 4, 8, P, None, 4, P, P, None, 8, 0, 1e-8, None) == EINVAL     # null x_max
            assert r(P, P, xt, yt, 4, 8, P, P, 4, None, P, None, 8, 0, 1e-8, None) == EINVAL     # null delta
            assert r(P, P, xt, yt, 4, 8, P, P, 4, P, None, None, 8, 0, 1e-8, None) == EINVAL     # asymmetric: zero_float
            assert r(P, P, xt, yt, 4, 8, P, P, 4, P, None, None, 8, 1, 1e-8, None) == EINVAL     # symmetric: the sign
            assert r(P, P, xt, yt, 4, 8, P, P, 2, P, P, None, 8, 0, 1e-8, None) == EINVAL        # n_range not in {1, C}
            assert r(P, P, xt, yt, 0, 8, P, P, 1, P, P, None, 8, 0, 1e-8, None) == EINVAL
            assert r(P, P, xt, yt, 4, 0, P, P, 1, P, P, None, 8, 0, 1e-8, None) == EINVAL
            assert r(P, P, xt, yt, 2, 1 << 31, P, P, 2, P, P, None, 8, 0, 1e-8, None) == EINVAL
            assert r(P, P, xt, yt, 4, 8, P, P, 4, P, P, None, 20, 0, 1e-8, None) == EUNSUPPORTED
            assert r(P, P, xt, yt, 4, 8, P, P, 1, P, None, P, 1, 1, 1e-8, None) == EUNSUPPORTED
        assert r(P, P, xt, 3 - xt, 4, 8, P, P, 4, P, P, None, 8, 0, 1e-8, None) == EINVAL
        assert r(P + 1, P, xt, xt, 4, 8, P, P, 4, P, P, None, 8, 0, 1e-8, None) == EINVAL
        assert r(P, P + 2, xt, F32, 4, 8, P, P, 4, P, P, None, 8, 0, 1e-8, None) == EINVAL
    for bad in (F32, 3, -1):
        assert r(P, P, bad, F32, 4, 8, P, P, 4, P, P, None, 8, 0, 1e-8, None) == EINVAL


def test_int_minmax_quantize_h16_argument_validation_without_gpu():
    import fp8q
    m = fp8q.lib().fp8q_int_minmax_quantize_h16
    # (x, y, x_type, y_type, C, inner, row_min, row_max, delta, zero_float, signed_flag, n_bits, symmetric, eps, ws, ws_bytes,
    #  stream)
    for xt in (F16, BF16):
        for yt in (F32, xt):
            assert m(None, P, xt, yt, 4, 8, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL
            assert m(P, None, xt, yt, 4, 8, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL
            assert m(P, P, xt, yt, 4, 8, None, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL   # null row_min
            assert m(P, P, xt, yt, 4, 8, P, None, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL   # null row_max
            assert m(P, P, xt, yt, 4, 8, P, P, None, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL   # null delta
            assert m(P, P, xt, yt, 4, 8, P, P, P, None, None, 8, 0, 1e-8, None, 0, None) == EINVAL
            assert m(P, P, xt, yt, 4, 8, P, P, P, None, None, 8, 1, 1e-8, None, 0, None) == EINVAL
            assert m(P, P, xt, yt, 0, 8, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL
            assert m(P, P, xt, yt, 4, 0, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL
            assert m(P, P, xt, yt, 4, 8, P, P, P, None, P, 1, 1, 1e-8, None, 0, None) == EUNSUPPORTED
            assert m(P, P, xt, yt, 4, 8, P, P, P, P, None, 17, 0, 1e-8, None, 0, None) == EUNSUPPORTED
            # long rows need the workspace of fp8q_minmax_workspace_bytes(C, inner), as fp8q_minmax_h16
            assert m(P, P, xt, yt, 2, 1 << 22, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EWORKSPACE
        assert m(P, P, xt, 3 - xt, 4, 8, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL
        assert m(P + 1, P, xt, xt, 4, 8, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL
    assert m(P, P, F32, F32, 4, 8, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == EINVAL


def test_int_wrappers_take_out_dtype_and_refuse_what_the_lane_does_not():
    import torch
    from fp8q import ops
    from fp8q._lib import Fp8qError
    d, z = torch.ones(1), torch.zeros(1)
    for dt in (torch.float16, torch.bfloat16):
        x = torch.zeros(4, 8, dtype=dt)
        other = torch.bfloat16 if dt == torch.float16 else torch.float16
        with pytest.raises(Fp8qError, match="CUDA"):                          # half x is accepted; there is no CPU path
            ops.int_quantize(x, d, z)
        with pytest.raises(Fp8qError, match="CUDA"):
            ops.int_range_quantize(x, d, d, out_dtype=dt)
        with pytest.raises(Fp8qError, match="CUDA"):
            ops.int_minmax_quantize(x, out_dtype=dt)
        for bad in (other, torch.float64, torch.int8):                        # float32 or x.dtype only
            with pytest.raises(Fp8qError, match="float32 or"):
                ops.int_quantize(x, d, z, out_dtype=bad)
            with pytest.raises(Fp8qError, match="float32 or"):
                ops.int_range_quantize(x, d, d, out_dtype=bad)
            with pytest.raises(Fp8qError, match="float32 or"):
                ops.int_minmax_quantize(x, out_dtype=bad)
        with pytest.raises(Fp8qError, match="float32 or"):
            ops.int_quantize(x, d, z, out=torch.empty(4, 8, dtype=other))
        with pytest.raises(Fp8qError, match="out_dtype"):                     # out and out_dtype disagree
            ops.int_quantize(x, d, z, out=torch.empty(4, 8, dtype=dt), out_dtype=torch.float32)
    with pytest.raises(Fp8qError, match="out_dtype"):                         # a float32 input gives a float32 result
        ops.int_quantize(torch.zeros(4), d, z, out_dtype=torch.bfloat16)


def test_uniform_quantizers_keep_dtype_option():
    import torch
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    from quantization.manager import QuantizationManager
    from quantization.quantization_manager import QMethods
    for cls in (AsymmetricUniformQuantizer, SymmetricUniformQuantizer):
        q, k = cls(n_bits=8), cls(n_bits=8, keep_dtype=True)
        assert q.keep_dtype is False and k.keep_dtype is True
        assert set(k.state_dict().keys()) == set(q.state_dict().keys())       # not part of the state dict
        # off CUDA the option changes nothing: the reference's op chain
        k.set_quant_range(torch.tensor(-1.0), torch.tensor(2.0))
        q.set_quant_range(torch.tensor(-1.0), torch.tensor(2.0))
        x = torch.linspace(-3, 3, 101)
        assert torch.equal(k(x), q(x))
    m = QuantizationManager(qmethod=QMethods.symmetric_uniform.cls, qparams=dict(n_bits=8, keep_dtype=True))
    assert m.quantizer.keep_dtype is True
