"""CPU-only checks of the uniform (INT) entry points of the C ABI (csrc/fp8q_int.hip): argument errors are reported
before any launch, so they are exercised without a GPU."""
import pytest


def test_int_argument_validation_without_gpu():
    import fp8q
    L = fp8q.lib()
    P = 4096                                     # a non-null pointer value that is never dereferenced (no launch)
    # fp8q_int_quantize_f32(x, y, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps, stream)
    q = L.fp8q_int_quantize_f32
    assert q(None, P, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == -1           # null x
    assert q(P, P, 4, 8, None, P, 1, None, 8, 0, 1e-8, None) == -1           # null delta
    assert q(P, P, 4, 8, P, None, 1, None, 8, 0, 1e-8, None) == -1           # asymmetric without zero_float
    assert q(P, P, 4, 8, P, None, 1, None, 8, 1, 1e-8, None) == -1           # symmetric without the sign
    assert q(P, P, 4, 8, P, P, 3, None, 8, 0, 1e-8, None) == -1              # n_delta not in {1, C}
    assert q(P, P, 0, 8, P, P, 1, None, 8, 0, 1e-8, None) == -1              # empty
    assert q(P, P, 4, -1, P, P, 1, None, 8, 0, 1e-8, None) == -1
    for nb in (1, 0, 17, 32):
        assert q(P, P, 4, 8, P, P, 4, None, nb, 0, 1e-8, None) == -2         # n_bits outside [2, 16]
        assert q(P, P, 4, 8, P, None, 1, P, nb, 1, 1e-8, None) == -2
    # fp8q_int_set_range_f32(x_min, x_max, n, delta, zero_float, signed_flag, n_bits, symmetric, eps, stream)
    s = L.fp8q_int_set_range_f32
    assert s(None, P, 4, P, P, None, 8, 0, 1e-8, None) == -1
    assert s(P, P, 0, P, P, None, 8, 0, 1e-8, None) == -1
    assert s(P, P, 4, P, P, None, 8, 1, 1e-8, None) == -1                    # symmetric without the sign
    assert s(P, P, 4, None, P, P, 8, 1, 1e-8, None) == -1
    assert s(P, P, 4, P, P, P, 1, 1, 1e-8, None) == -2
    assert s(P, P, 4, P, P, None, 17, 0, 1e-8, None) == -2
    # fp8q_int_range_quantize_f32(x, y, C, inner, x_min, x_max, n_range, delta, zero_float, signed_flag, n_bits,
    #                             symmetric, eps, stream)
    r = L.fp8q_int_range_quantize_f32
    assert r(P, None, 4, 8, P, P, 4, P, P, None, 8, 0, 1e-8, None) == -1
    assert r(P, P, 4, 8, P, P, 2, P, P, None, 8, 0, 1e-8, None) == -1
    assert r(P, P, 4, 8, None, P, 4, P, P, None, 8, 0, 1e-8, None) == -1
    assert r(P, P, 4, 8, P, P, 4, P, P, None, 20, 0, 1e-8, None) == -2
    # fp8q_int_minmax_quantize_f32(x, y, C, inner, row_min, row_max, delta, zero_float, signed_flag, n_bits,
    #                              symmetric, eps, ws, ws_bytes, stream)
    m = L.fp8q_int_minmax_quantize_f32
    assert m(P, P, 4, 8, None, P, P, P, None, 8, 0, 1e-8, None, 0, None) == -1
    assert m(P, P, 0, 8, P, P, P, P, None, 8, 0, 1e-8, None, 0, None) == -1
    assert m(P, P, 4, 8, P, P, P, None, P, 1, 1, 1e-8, None, 0, None) == -2


def test_int_wrappers_refuse_cpu_tensors():
    import torch
    from fp8q import ops
    from fp8q._lib import Fp8qError
    with pytest.raises(Fp8qError):
        ops.int_quantize(torch.zeros(4), torch.ones(1), torch.zeros(1))
    with pytest.raises(Fp8qError):
        ops.int_set_range(torch.zeros(1), torch.ones(1))


def test_cpu_quantizers_stay_on_the_eager_chain():
    """Off CUDA the reference's op chain runs as before (and the range epoch follows every assignment)."""
    import torch
    from quantization.uniform import SymmetricUniformQuantizer, AsymmetricUniformQuantizer
    q = SymmetricUniformQuantizer(n_bits=8)
    e0 = getattr(q, "_range_epoch", 0)
    q.set_quant_range(torch.tensor(-1.0), torch.tensor(2.0))
    assert q._range_epoch > e0 and q._signed.dtype == torch.bool and q._signed.dim() == 0
    x = torch.linspace(-3, 3, 101)
    want = torch.clamp(torch.round(x / q._delta), -128, 127) * q._delta
    assert torch.equal(q(x), want)
    a = AsymmetricUniformQuantizer(n_bits=4, per_channel=True)
    a.set_quant_range(torch.tensor([-1.0, 0.5]), torch.tensor([1.0, 2.0]))
    e1 = a._range_epoch
    a.load_state_dict(a.state_dict())
    assert a._range_epoch > e1
