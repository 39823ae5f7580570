"""CPU-only checks of the INT fused-epilogue entry points of the C ABI (csrc/fp8q_intepilogue.hip): both symbols are
exported and bound, and argument errors are reported before any launch, so they are exercised without a GPU."""
import pytest

NAMES = ("fp8q_int_affine_act_quantize_f32", "fp8q_int_affine_act_range_quantize_f32")


def test_symbols_are_exported_and_bound():
    import fp8q
    from fp8q._lib import SIGNATURES
    L = fp8q.lib()
    for name in NAMES:
        assert name in SIGNATURES
        fn = getattr(L, name)
        assert fn.argtypes == SIGNATURES[name][1] and fn.restype is SIGNATURES[name][0]


def test_argument_validation_without_gpu():
    import fp8q
    L = fp8q.lib()
    P = 4096                                     # a non-null, 16-byte aligned pointer value that is never dereferenced
    # (x, residual, y, N, C, HW, alpha_beta, act, delta, zero_float, signed_flag, n_bits, symmetric, eps, stream)
    q = L.fp8q_int_affine_act_quantize_f32
    assert q(None, None, P, 2, 8, 4, P, 1, P, P, None, 8, 0, 1e-8, None) == -1         # null x
    assert q(P, None, None, 2, 8, 4, P, 1, P, P, None, 8, 0, 1e-8, None) == -1         # null y
    assert q(P, None, P, 2, 8, 4, P, 1, None, P, None, 8, 0, 1e-8, None) == -1         # null delta
    assert q(P, None, P, 2, 8, 4, P, 1, P, None, None, 8, 0, 1e-8, None) == -1         # asymmetric without zero_float
    assert q(P, None, P, 2, 8, 4, P, 1, P, None, None, 8, 1, 1e-8, None) == -1         # symmetric without the sign
    assert q(P, None, P, 2, 8, 4, P, 3, P, P, None, 8, 0, 1e-8, None) == -1            # act = 3
    assert q(P, None, P, 2, 8, 4, P, -1, P, P, None, 8, 0, 1e-8, None) == -1
    assert q(P, None, P, 2, 0, 4, P, 1, P, P, None, 8, 0, 1e-8, None) == -1            # C = 0
    assert q(P, None, P, -1, 8, 4, P, 1, P, P, None, 8, 0, 1e-8, None) == -1
    assert q(P + 4, None, P, 2, 8, 4, P, 1, P, P, None, 8, 0, 1e-8, None) == -1        # x off its 16-byte boundary
    assert q(P, P + 8, P, 2, 8, 4, P, 1, P, P, None, 8, 0, 1e-8, None) == -1           # residual
    assert q(P, None, P + 4, 2, 8, 4, P, 1, P, P, None, 8, 0, 1e-8, None) == -1        # y
    assert q(P, None, P, 2, 8, 4, P + 4, 1, P, P, None, 8, 0, 1e-8, None) == -1        # alpha_beta off its 8-byte boundary
    assert q(P, None, P, 2, 8, 4, P, 1, P + 2, P, None, 8, 0, 1e-8, None) == -1        # delta off its 4-byte boundary
    for nb in (1, 17):
        assert q(P, None, P, 2, 8, 4, P, 1, P, P, None, nb, 0, 1e-8, None) == -2       # n_bits outside [2, 16]
        assert q(P, None, P, 2, 8, 4, P, 1, P, None, P, nb, 1, 1e-8, None) == -2
    assert q(P, None, P, 2, 3, 25, None, 0, P, P, None, 8, 0, 1e-8, None) == -2        # C*HW = 75
    assert q(P, None, P, 2, 1 << 20, 1 << 12, None, 0, P, P, None, 8, 0, 1e-8, None) == -2   # C*HW >= 2^31
    assert q(None, None, None, 0, 8, 4, None, 0, None, None, None, 8, 0, 1e-8, None) == 0    # N = 0: nothing to do
    # (x, residual, y, N, C, HW, alpha_beta, act, x_min, x_max, delta_out, zero_float_out, signed_flag_out, n_bits,
    #  symmetric, eps, stream)
    r = L.fp8q_int_affine_act_range_quantize_f32
    assert r(None, None, P, 2, 8, 4, P, 1, P, P, P, P, None, 8, 0, 1e-8, None) == -1
    assert r(P, None, P, 2, 8, 4, P, 1, None, P, P, P, None, 8, 0, 1e-8, None) == -1   # null x_min
    assert r(P, None, P, 2, 8, 4, P, 1, P, None, P, P, None, 8, 0, 1e-8, None) == -1   # null x_max
    assert r(P, None, P, 2, 8, 4, P, 1, P, None, P, None, P, 8, 1, 1e-8, None) == -1   # ... symmetric too
    assert r(P, None, P, 2, 8, 4, P, 1, P, P, None, P, None, 8, 0, 1e-8, None) == -1   # null delta_out
    assert r(P, None, P, 2, 8, 4, P, 1, P, P, P, None, None, 8, 0, 1e-8, None) == -1   # asymmetric without zero_float_out
    assert r(P, None, P, 2, 8, 4, P, 1, P, P, P, None, None, 8, 1, 1e-8, None) == -1   # symmetric without the sign
    assert r(P, None, P, 2, 8, 4, P, 3, P, P, P, P, None, 8, 0, 1e-8, None) == -1
    assert r(P, None, P + 4, 2, 8, 4, P, 1, P, P, P, P, None, 8, 0, 1e-8, None) == -1
    assert r(P, None, P, 2, 8, 4, P, 1, P, P, P, P, None, 1, 0, 1e-8, None) == -2
    assert r(P, None, P, 2, 8, 4, P, 1, P, P, P, None, P, 17, 1, 1e-8, None) == -2
    assert r(P, None, P, 2, 3, 25, P, 1, P, P, P, P, None, 8, 0, 1e-8, None) == -2
    assert r(None, None, None, 0, 8, 4, None, 0, None, None, None, None, None, 8, 0, 1e-8, None) == 0


def test_wrappers_refuse_cpu_tensors():
    import torch
    from fp8q import ops
    from fp8q._lib import Fp8qError
    x = torch.zeros(2, 4, 2, 2)
    with pytest.raises(Fp8qError):
        ops.int_affine_act_quantize(x, torch.ones(1), torch.zeros(1), None, 8, False, 1e-8)
    with pytest.raises(Fp8qError):
        ops.int_affine_act_range_quantize(x, torch.zeros(1), torch.ones(1), 8, True, 1e-8)


def test_fuse_epilogue_is_a_constructor_setting_not_state():
    import torch
    from quantization.uniform import SymmetricUniformQuantizer, AsymmetricUniformQuantizer
    for cls in (SymmetricUniformQuantizer, AsymmetricUniformQuantizer):
        assert cls(n_bits=8).fuse_epilogue is False
        q = cls(n_bits=8, fuse_epilogue=True)
        assert q.fuse_epilogue is True
        q.set_quant_range(torch.tensor(-1.0), torch.tensor(2.0))
        assert not any("fuse" in k for k in q.state_dict())
