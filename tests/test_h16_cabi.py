"""CPU-only checks of the half-precision entry points of the C ABI (csrc/fp8q_h16.hip): every argument error is
reported before any launch, so it is exercised without a GPU; the ops wrappers refuse what the lane does not take."""
import pytest

F32, F16, BF16 = 0, 1, 2
EINVAL, EUNSUPPORTED, EWORKSPACE, ETOOLONG = -1, -2, -3, -4
P = 4096                                     # a non-null, even pointer value that is never dereferenced (no launch)


def test_h16_constants_in_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fp8q.h")).read()
    for name, val in (("FP8Q_DT_F32", F32), ("FP8Q_DT_F16", F16), ("FP8Q_DT_BF16", BF16)):
        assert re.search(rf"#define {name} {val}\b", hdr)
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr)


def test_quantize_h16_argument_validation_without_gpu():
    import fp8q
    q = fp8q.lib().fp8q_quantize_h16
    # (x, y, x_type, y_type, C, inner, maxval, n_maxval, mbits, n_bits, sign_bits, stream)
    for xt in (F16, BF16):
        assert q(None, P, xt, F32, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL       # null x
        assert q(P, None, xt, F32, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL       # null y
        assert q(P, P, xt, xt, 4, 8, None, 1, 3.0, 8, 1, None) == EINVAL        # null maxval
        assert q(P, P, xt, F32, 4, 8, P, 3, 3.0, 8, 1, None) == EINVAL          # n_maxval not in {1, C}
        assert q(P, P, xt, F32, 0, 8, P, 1, 3.0, 8, 1, None) == EINVAL          # empty
        assert q(P, P, xt, F32, 4, 0, P, 1, 3.0, 8, 1, None) == EINVAL
        assert q(P, P, xt, F32, 4, -1, P, 1, 3.0, 8, 1, None) == EINVAL
        assert q(P, P, xt, 3 - xt, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL       # y_type: the OTHER half type
        assert q(P, P, xt, 7, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL
        assert q(P + 1, P, xt, xt, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL       # odd address of a 2-byte element
        assert q(P, P + 2, xt, F32, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL      # fp32 output at a 2-byte phase
        assert q(P, P, xt, xt, 4, 8, P, 1, 3.0, 8, 2, None) == EINVAL           # sign_bits not in {0, 1}
        assert q(P, P, xt, xt, 4, 8, P, 4, 1.0, 16, 1, None) == EUNSUPPORTED    # 14 exponent bits
        assert q(P, P, xt, F32, 4, 8, P, 1, 1.0, 10, 1, None) == EUNSUPPORTED   # 8 exponent bits
    for bad in (F32, 3, -1):                                                    # x_type is not a half type
        assert q(P, P, bad, F32, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL


def test_minmax_h16_argument_validation_without_gpu():
    import fp8q
    m = fp8q.lib().fp8q_minmax_h16
    # (x, x_type, C, inner, cur_min, cur_max, maxval_out, fold_mode, momentum, first, ws, ws_bytes, stream)
    for xt in (F16, BF16):
        assert m(None, xt, 1, 8, P, P, None, 0, 0.9, 1, P, 1 << 16, None) == EINVAL
        assert m(P, xt, 1, 8, None, P, None, 0, 0.9, 1, P, 1 << 16, None) == EINVAL
        assert m(P, xt, 1, 8, P, None, None, 0, 0.9, 1, P, 1 << 16, None) == EINVAL
        assert m(P, xt, 0, 8, P, P, None, 0, 0.9, 1, P, 1 << 16, None) == EINVAL       # empty
        assert m(P, xt, 1, 0, P, P, None, 0, 0.9, 1, P, 1 << 16, None) == EINVAL
        assert m(P, xt, 1, 8, P, P, None, 3, 0.9, 1, P, 1 << 16, None) == EINVAL       # unknown fold mode
        assert m(P, xt, 1, 8, P, P, None, -1, 0.9, 1, P, 1 << 16, None) == EINVAL
        assert m(P + 1, xt, 1, 8, P, P, None, 0, 0.9, 1, P, 1 << 16, None) == EINVAL
        # per tensor / long rows need the workspace of fp8q_minmax_workspace_bytes(C, inner)
        assert m(P, xt, 1, 1 << 22, P, P, None, 0, 0.9, 1, None, 0, None) == EWORKSPACE
        assert m(P, xt, 1, 1 << 22, P, P, None, 0, 0.9, 1, P, 8, None) == EWORKSPACE
        assert m(P, xt, 1, 1 << 22, P, P, None, 0, 0.9, 1, P + 4, 1 << 20, None) == EWORKSPACE   # misaligned
    for bad in (F32, 3, -1):
        assert m(P, bad, 1, 8, P, P, None, 0, 0.9, 1, P, 1 << 16, None) == EINVAL


def test_minmax_quantize_h16_argument_validation_without_gpu():
    import fp8q
    L = fp8q.lib()
    f = L.fp8q_minmax_quantize_h16
    # (x, y, x_type, y_type, C, inner, row_min, row_max, maxval_out, mbits, n_bits, sign_bits, stream)
    for xt in (F16, BF16):
        assert f(None, P, xt, F32, 4, 8, P, P, P, 3.0, 8, 1, None) == EINVAL
        assert f(P, None, xt, xt, 4, 8, P, P, P, 3.0, 8, 1, None) == EINVAL
        assert f(P, P, xt, xt, 4, 8, P, P, None, 3.0, 8, 1, None) == EINVAL            # maxval_out carries the ranges
        assert f(P, P, xt, xt, 0, 8, P, P, P, 3.0, 8, 1, None) == EINVAL
        assert f(P, P, xt, xt, 4, 0, P, P, P, 3.0, 8, 1, None) == EINVAL
        assert f(P, P, xt, 3 - xt, 4, 8, P, P, P, 3.0, 8, 1, None) == EINVAL
        assert f(P, P, xt, xt, 4, 8, P, P, P, 1.0, 16, 1, None) == EUNSUPPORTED
        assert f(P, P, xt, xt, 4, L.fp8q_fused_max_inner() + 1, P, P, P, 3.0, 8, 1, None) == ETOOLONG
    assert f(P, P, F32, F32, 4, 8, P, P, P, 3.0, 8, 1, None) == EINVAL


def test_h16_wrappers_refuse_what_the_lane_does_not_take():
    import torch
    from fp8q import ops
    from fp8q._lib import Fp8qError
    mv = torch.ones(1)
    for dt in (torch.float16, torch.bfloat16):
        x = torch.zeros(4, 8, dtype=dt)
        other = torch.bfloat16 if dt == torch.float16 else torch.float16
        with pytest.raises(Fp8qError, match="CUDA"):                          # no CPU path
            ops.quantize(x, mv, 3.0)
        with pytest.raises(Fp8qError, match="CUDA"):
            ops.minmax(x, False)
        with pytest.raises(Fp8qError, match="CUDA"):
            ops.minmax_quantize(x, 3.0)
        for bad in (other, torch.float64, torch.int8):                        # float32 or x.dtype only
            with pytest.raises(Fp8qError, match="float32 or"):
                ops.quantize(x, mv, 3.0, out_dtype=bad)
            with pytest.raises(Fp8qError, match="float32 or"):
                ops.minmax_quantize(x, 3.0, out_dtype=bad)
        with pytest.raises(Fp8qError, match="float32 or"):
            ops.quantize(x, mv, 3.0, out=torch.empty(4, 8, dtype=other))
        with pytest.raises(Fp8qError, match="float32-only"):                  # device-resident width / sign: fp32 lane only
            ops.quantize(x, mv, torch.tensor([3.0]))
        with pytest.raises(Fp8qError, match="float32-only"):
            ops.quantize(x, mv, 3.0, sign_bits=torch.ones(1, dtype=torch.uint8))
        with pytest.raises(Fp8qError, match="float32-only"):                  # packed data-parallel ranges
            ops.minmax(x, False, packed=torch.empty(1, 4))


def test_fpquantizer_keep_dtype_option():
    from quantization.fp8 import FPQuantizer
    q = FPQuantizer(n_bits=8, mantissa_bits=3)
    assert q.keep_dtype is False
    k = FPQuantizer(n_bits=8, mantissa_bits=3, keep_dtype=True)
    assert k.keep_dtype is True
    assert set(k.state_dict().keys()) == set(q.state_dict().keys())           # not part of the state dict
