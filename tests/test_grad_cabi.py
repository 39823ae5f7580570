"""CPU-only checks of the backward entry points of the C ABI (csrc/fp8q_grad.hip): the symbols and their prototypes, every
argument error (reported before any launch, so exercised without a GPU), the workspace size, and what the ops wrapper
refuses."""
import os
import re

import pytest

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
P = 4096                                     # a non-null, aligned pointer value that is never dereferenced (no launch)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_prototypes():
    import fp8q
    L = fp8q.lib()
    assert hasattr(L, "fp8q_quantize_bwd_f32") and hasattr(L, "fp8q_quantize_bwd_workspace_bytes")
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fp8q.h")).read())
    assert ("int fp8q_quantize_bwd_f32(const float *x, const float *g, float *gx, int64_t C, int64_t inner, "
            "const float *maxval, int64_t n_maxval, float mbits, const float *mbits_dev, int n_bits, int sign_bits, "
            "float *gmaxval, float *gmbits, void *ws, size_t ws_bytes, fp8q_stream_t stream);") in hdr
    assert "size_t fp8q_quantize_bwd_workspace_bytes(int64_t C, int64_t inner, int64_t n_maxval);" in hdr
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr)                       # additive entries
    from fp8q import build
    assert "fp8q_grad.hip" in build.SOURCES


def test_argument_validation_without_gpu():
    import fp8q
    L = fp8q.lib()
    f = L.fp8q_quantize_bwd_f32
    W = 1 << 20
    # (x, g, gx, C, inner, maxval, n_maxval, mbits, mbits_dev, n_bits, sign_bits, gmaxval, gmbits, ws, ws_bytes, stream)
    assert f(None, P, P, 4, 8, P, 1, 3.0, None, 8, 1, P, P, P, W, None) == EINVAL        # null x
    assert f(P, None, P, 4, 8, P, 1, 3.0, None, 8, 1, P, P, P, W, None) == EINVAL        # null g
    assert f(P, P, P, 4, 8, None, 1, 3.0, None, 8, 1, P, P, P, W, None) == EINVAL        # null maxval
    assert f(P, P, P, 0, 8, P, 1, 3.0, None, 8, 1, P, P, P, W, None) == EINVAL           # empty
    assert f(P, P, P, 4, 0, P, 1, 3.0, None, 8, 1, P, P, P, W, None) == EINVAL
    assert f(P, P, P, 4, -1, P, 1, 3.0, None, 8, 1, P, P, P, W, None) == EINVAL
    assert f(P, P, P, 4, 8, P, 3, 3.0, None, 8, 1, P, P, P, W, None) == EINVAL           # n_maxval not in {1, C}
    assert f(P, P, P, 4, 8, P, 1, 3.0, None, 8, 2, P, P, P, W, None) == EINVAL           # sign_bits not in {0, 1}
    assert f(P, P, P, 4, 8, P, 1, 3.0, None, 8, -1, P, P, P, W, None) == EINVAL
    assert f(P, P, None, 4, 8, P, 1, 3.0, None, 8, 1, None, None, P, W, None) == EINVAL  # nothing requested
    for k in range(7):                                                                   # misaligned fp32 pointers
        a = [P, P, P, 4, 8, P, 1, 3.0, P, 8, 1, P, P, P, W, None]
        a[(0, 1, 2, 5, 8, 11, 12)[k]] = P + 2
        assert f(*a) == EINVAL, k
    assert f(P, P, P, 4, 8, P, 1, float("nan"), None, 8, 1, P, P, P, W, None) == EINVAL  # as the forward
    # the formats the forward refuses
    assert f(P, P, P, 4, 8, P, 4, 1.0, None, 16, 1, P, P, P, W, None) == EUNSUPPORTED    # 14 exponent bits
    assert f(P, P, P, 4, 8, P, 1, 1.0, None, 10, 1, P, P, P, W, None) == EUNSUPPORTED    # 8 exponent bits
    assert f(P, P, P, 4, 8, P, 1, 0.0, P, 10, 1, P, P, P, W, None) == EUNSUPPORTED       # device width: M = 1 is admitted
    # workspace: needed for the sums, not for gx alone
    need = L.fp8q_quantize_bwd_workspace_bytes(1, 1 << 22, 1)
    assert f(P, P, P, 1, 1 << 22, P, 1, 3.0, None, 8, 1, P, None, None, 0, None) == EWORKSPACE
    assert f(P, P, P, 1, 1 << 22, P, 1, 3.0, None, 8, 1, None, P, P, need - 8, None) == EWORKSPACE
    assert f(P, P, P, 1, 1 << 22, P, 1, 3.0, None, 8, 1, P, P, P + 4, W, None) == EWORKSPACE      # misaligned
    # argument errors come before the workspace error
    assert f(None, P, P, 1, 1 << 22, P, 1, 3.0, None, 8, 1, P, P, None, 0, None) == EINVAL


def test_workspace_bytes():
    import fp8q
    ws = fp8q.lib().fp8q_quantize_bwd_workspace_bytes
    assert ws(1, 1 << 22, 1) > 0 and ws(1, 300_000_000, 1) > 0           # a split row
    assert ws(1 << 21, 147, 1 << 21) >= 16 * (1 << 21) // 256            # many short rows: a partial per block at least
    assert ws(0, 8, 1) == 0 and ws(4, 8, 3) == 0                         # (shapes the entry point refuses)
    shapes = [(1, 1), (1, 9), (1, 4097), (3, 4097), (64, 147), (64, 4099), (96, 9), (1 << 16, 27), (1 << 21, 147),
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
    x, mv = torch.zeros(4, 8), torch.ones(1)
    with pytest.raises(Fp8qError, match="CUDA"):                              # no CPU path
        ops.quantize_backward(x, x, mv, 3.0)
    with pytest.raises(Fp8qError, match="CUDA"):
        ops.quantize_backward(x.double(), x.double(), mv, 3.0)


def test_env_switch_and_cpu_route_keep_the_torch_chain(monkeypatch):
    """CPU tensors (the oracle backend) never reach ops.quantize_backward"""
    import torch
    import oracle_ops
    from fp8q import ops
    from quantization.fp8 import FPQuantizer, _grad_kernels
    assert _grad_kernels()
    monkeypatch.setenv("FP8Q_GRAD_KERNELS", "0")
    assert not _grad_kernels()
    monkeypatch.delenv("FP8Q_GRAD_KERNELS")
    calls = []
    monkeypatch.setattr(ops, "quantize_backward", lambda *a, **k: calls.append(a))
    q = FPQuantizer(n_bits=8, mantissa_bits=3, maxval=1.5)
    q.learn_maxval()
    with oracle_ops.patched():
        q(torch.randn(4, 16) * 2).sum().backward()
    assert not calls and q.maxval.grad is not None
