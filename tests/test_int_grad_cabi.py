"""CPU-only checks of the INT backward entry points of the C ABI (csrc/fp8q_intgrad.hip): the symbols and their prototypes,
every argument error (reported before any launch, so exercised without a GPU), the workspace size, what the ops wrapper
refuses, and the CPU route of the quantizers (the torch chain, now with LSQ's gradient scaling)."""
import os
import re

import pytest

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
P = 4096                                     # a non-null, aligned pointer value that is never dereferenced (no launch)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_prototypes():
    import fp8q
    L = fp8q.lib()
    assert hasattr(L, "fp8q_int_quantize_bwd_f32") and hasattr(L, "fp8q_int_quantize_bwd_workspace_bytes")
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fp8q.h")).read())
    assert ("int fp8q_int_quantize_bwd_f32(const float *x, const float *g, float *gx, int64_t C, int64_t inner, "
            "const float *delta, const float *zero_float, int64_t n_delta, const unsigned char *signed_flag, int n_bits, "
            "int symmetric, float eps, int64_t grad_scale_elems, float *gdelta, float *gzero_float, void *ws, "
            "size_t ws_bytes, fp8q_stream_t stream);") in hdr
    assert "size_t fp8q_int_quantize_bwd_workspace_bytes(int64_t C, int64_t inner, int64_t n_delta);" in hdr
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr)                       # additive entries
    from fp8q import build
    assert "fp8q_intgrad.hip" in build.SOURCES


def _args(**kw):
    """a valid asymmetric call: (x, g, gx, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps,
    grad_scale_elems, gdelta, gzero_float, ws, ws_bytes, stream)"""
    a = dict(x=P, g=P, gx=P, C=4, inner=8, delta=P, zero_float=P, n_delta=1, signed_flag=None, n_bits=8, symmetric=0,
             eps=1e-8, grad_scale_elems=0, gdelta=P, gzero_float=P, ws=P, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return list(a.values())


def test_argument_validation_without_gpu():
    import fp8q
    L = fp8q.lib()
    f = L.fp8q_int_quantize_bwd_f32
    sym = dict(symmetric=1, signed_flag=P, zero_float=None, gzero_float=None)
    for bad in (dict(x=None), dict(g=None), dict(delta=None),
                dict(zero_float=None),                                          # asymmetric without zero_float
                dict(sym, signed_flag=None),                                    # symmetric without the sign
                dict(C=0), dict(inner=0), dict(inner=-1), dict(C=-3),           # empty
                dict(n_delta=3), dict(n_delta=0), dict(n_delta=8),              # n_delta not in {1, C}
                dict(gx=None, gdelta=None, gzero_float=None),                   # nothing requested
                dict(sym, gzero_float=P),                                       # a symmetric quantizer has no zero_float
                dict(grad_scale_elems=-1)):
        assert f(*_args(**bad)) == EINVAL, bad
    for name in ("x", "g", "gx", "delta", "zero_float", "gdelta", "gzero_float"):            # misaligned fp32 pointers
        assert f(*_args(**{name: P + 2})) == EINVAL, name
    for nb in (1, 0, -4, 17, 32):
        assert f(*_args(n_bits=nb)) == EUNSUPPORTED                             # n_bits outside [2, 16]
        assert f(*_args(n_bits=nb, n_delta=4)) == EUNSUPPORTED
        assert f(*_args(**dict(sym, n_bits=nb))) == EUNSUPPORTED
    # workspace: needed for the sums, not for gx alone
    big = dict(C=1, inner=1 << 22)
    need = L.fp8q_int_quantize_bwd_workspace_bytes(1, 1 << 22, 1)
    assert need > 0
    assert f(*_args(**big, ws=None, ws_bytes=0)) == EWORKSPACE
    assert f(*_args(**big, gdelta=None, ws_bytes=need - 8)) == EWORKSPACE
    assert f(*_args(**big, gzero_float=None, ws_bytes=need - 8)) == EWORKSPACE
    assert f(*_args(**big, ws=P + 4)) == EWORKSPACE                             # misaligned
    assert f(*_args(**dict(sym, **big), ws=None, ws_bytes=0)) == EWORKSPACE
    # argument errors come before the workspace error
    assert f(*_args(**big, x=None, ws=None, ws_bytes=0)) == EINVAL
    assert f(*_args(**big, n_bits=17, ws=None, ws_bytes=0)) == EUNSUPPORTED


def test_workspace_bytes():
    import fp8q
    ws = fp8q.lib().fp8q_int_quantize_bwd_workspace_bytes
    assert ws(1, 1 << 22, 1) > 0 and ws(1, 300_000_000, 1) > 0           # a split row
    assert ws(0, 8, 1) == 0 and ws(4, 8, 3) == 0                         # (shapes the entry point refuses)
    shapes = [(1, 1), (1, 9), (1, 4097), (3, 4097), (64, 147), (64, 4099), (96, 9), (70000, 5), (1 << 21, 147),
              (1, (1 << 24) + 5), (8, 1 << 22), (1, 300_000_000)]
    for C, inner in shapes:
        for C2, inner2 in shapes:
            if C <= C2 and inner <= inner2:
                assert ws(C, inner, 1) <= ws(C2, inner2, 1), (C, inner, C2, inner2)
                assert ws(C, inner, C) <= ws(C2, inner2, C2), (C, inner, C2, inner2)
        assert ws(C, inner, 1) <= ws(C, inner, C)
        assert ws(C, inner, C) % 8 == 0


def test_wrapper_refuses_what_the_kernel_does_not_take():
    import torch
    from fp8q import ops
    from fp8q._lib import Fp8qError
    x, d = torch.zeros(4, 8), torch.ones(1)
    with pytest.raises(Fp8qError, match="CUDA"):                              # no CPU path
        ops.int_quantize_backward(x, x, d, torch.zeros(1))
    with pytest.raises(Fp8qError, match="CUDA"):
        ops.int_quantize_backward(x.double(), x.double(), d, torch.zeros(1))


@pytest.mark.parametrize("symmetric", [False, True])
def test_cpu_route_keeps_the_torch_chain_and_honours_grad_scaling(symmetric, monkeypatch):
    """CPU tensors never reach ops.int_quantize_backward; grad_scaling multiplies the range gradients by
    1 / sqrt(int_max * N) and nothing else"""
    import torch
    from fp8q import ops
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    calls = []
    monkeypatch.setattr(ops, "int_quantize_backward", lambda *a, **k: calls.append(a))
    cls = SymmetricUniformQuantizer if symmetric else AsymmetricUniformQuantizer
    torch.manual_seed(0)
    x0 = torch.randn(6, 40) * 2
    up = torch.randn(6, 40)
    res = {}
    for scaling in (False, True):
        q = cls(n_bits=4, per_channel=True, grad_scaling=scaling)
        q.set_quant_range(x0.min(1).values * 0.7, x0.max(1).values * 0.7)
        q.make_range_trainable()
        x = x0.clone().requires_grad_(True)
        y = q(x)
        y.backward(up)
        res[scaling] = (y.detach(), x.grad, q._delta.grad, None if symmetric else q._zero_float.grad)
    assert not calls
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    gs = (q.int_max * 40) ** -0.5
    assert q.calculate_grad_scale(x0) == gs
    for plain, scaled in zip(res[False][2:], res[True][2:]):
        if plain is not None:
            assert float(plain.abs().sum()) > 0
            # two scaled branches summed against one scaled sum: fp32 roundings of a 40-term sum that may cancel
            torch.testing.assert_close(scaled, plain * gs, rtol=1e-5, atol=1e-5 * gs * float(plain.abs().max()))
