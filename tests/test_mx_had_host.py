"""CPU-only checks of the MX lane's block Hadamard rotation (the fp8q_mxh_* entries, ops.hadamard32, hadamard= on the mx_* ops):
the reference the GPU tests compare with -- the contract of include/fp8q.h in ten lines of torch -- against the matrix form in
float64, the constant, the C ABI's table, and the argument refusals that need no device."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = torch.tensor(2.0 ** -2.5, dtype=torch.float32)
ENTRIES = {"transform": 7, "encode": 12, "quantize": 11, "encode_t": 12, "quantize_t": 11}      # arguments of the _f32 form


def ref_had(x, mask, inverse=False):
    """the rotation of every block of 32 along the last dimension of x (float32, CPU) as the contract reads: the sign multiply,
    five stages of (a + b, a - b) on float32, one multiplication by the float32 c; the inverse takes the signs last"""
    sg = torch.tensor([-1.0 if mask >> i & 1 else 1.0 for i in range(32)])
    v = x.reshape(-1, 32)
    v = v if inverse else v * sg
    for s in range(5):
        v = v.reshape(-1, 16 >> s, 2, 1 << s)
        v = torch.stack((v[:, :, 0] + v[:, :, 1], v[:, :, 0] - v[:, :, 1]), 2)
    v = v.reshape(-1, 32) * C
    return (v * sg if inverse else v).reshape(x.shape)


def test_reference_against_the_matrix_form():
    """|ref - x H / sqrt(32)| <= 7 * 2^-24 * 2^-2.5 * sum |x_i| per block: five rounded additions on the way to each output,
    the rounded product, and c's own rounding, each at most 2^-24 relative to a partial sum of magnitudes"""
    i = torch.arange(32)
    H = torch.tensor([[(-1.0) ** bin(int(a & b)).count("1") for b in i] for a in i], dtype=torch.float64)
    x = torch.randn(64, 32, generator=torch.Generator().manual_seed(0))
    for mask in (0, 0x80000001, 0xDEADBEEF):
        sg = torch.tensor([-1.0 if mask >> k & 1 else 1.0 for k in range(32)], dtype=torch.float64)
        bound = 7 * 2.0 ** -24 * 2.0 ** -2.5 * x.double().abs().sum(1, keepdim=True)
        assert ((ref_had(x, mask).double() - (x.double() * sg) @ H / 32 ** 0.5).abs() <= bound).all()
        assert ((ref_had(x, mask, inverse=True).double() - (x.double() @ H / 32 ** 0.5) * sg).abs() <= bound).all()
        assert torch.allclose(ref_had(ref_had(x, mask), mask, inverse=True), x, atol=1e-5)


def test_constant_and_signed_zeros():
    assert C.view(torch.int32).item() == 0x3E3504F3
    for val, negatives in ((1.5, 0), (-1.5, 1)):        # outputs 1 .. 31 are lower - upper: +0, which -(upper - lower) is not
        y = ref_had(torch.full((32,), val), 0)
        assert (y[1:] == 0).all() and int((y.view(torch.int32) < 0).sum()) == negatives


def test_entries_and_version():
    from fp8q import _lib, build
    names = [f"fp8q_mxh_{op}_{sfx}" for op in ENTRIES for sfx in ("f32", "h16")]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("fp8q_mxh_")) == sorted(names)
    for op, n in ENTRIES.items():
        f32, h16 = _lib.SIGNATURES[f"fp8q_mxh_{op}_f32"][1], _lib.SIGNATURES[f"fp8q_mxh_{op}_h16"][1]
        assert len(f32) == n and len(h16) == n + (1 if op.startswith("encode") else 2)
    hdr = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr) and "0x3E3504F3" in hdr
    assert {"fp8q_mx_had.hip", "fp8q_mx_had_t.hip"} <= set(build.SOURCES) and "fp8q_hadq.h" in build.HEADERS


def test_c_refusals_before_the_launch():
    import fp8q
    L = fp8q.lib()
    p = 4096                                                    # a made-up aligned address: nothing is launched
    assert L.fp8q_mxh_transform_f32(p, p, 2, 48, 0, 0, None) == -1                        # K % 32
    assert L.fp8q_mxh_transform_h16(p, p, 0, 0, 2, 64, 0, 0, None) == -1                  # no half side
    assert L.fp8q_mxh_encode_f32(p, p, p, 2, 33, 0, 0, 0, 0, 0, 0, None) == -1
    assert L.fp8q_mxh_encode_f32(p, p, p, 2, 64, 3, 0, 0, 0, 0, 0, None) == -2            # format 3 is unassigned
    assert L.fp8q_mxh_quantize_f32(p, p, 2, 64, 0, 0, 0, 2, 0, 0, None) == -1             # sr is 0 or 1
    assert L.fp8q_mxh_quantize_f32(p, p, 2, 64, 0, 0, 0, 1, 5, 4, None) == -1             # offset % 8
    assert L.fp8q_mxh_encode_t_f32(p, p, p, 48, 64, 0, 0, 0, 0, 0, 0, None) == -1         # R % 32
    assert L.fp8q_mxh_quantize_t_h16(p, p, 1, 2, 64, 64, 0, 0, 0, 0, 0, 0, None) == -1    # float16 in, bfloat16 out


@pytest.mark.parametrize("bad", [True, -1, 1 << 32, 1.0, "1"])
def test_python_refusals(bad):
    from fp8q import ops
    from quantization.mx import MXQuantizer
    x = torch.zeros(32, 64)
    for op in (ops.mx_encode, ops.mx_quantize, ops.mx_encode_t, ops.mx_quantize_t):
        with pytest.raises(ValueError):
            op(x, torch.float8_e4m3fn, hadamard=bad)
    with pytest.raises(ValueError):
        ops.hadamard32(x, bad)
    with pytest.raises(ValueError):
        MXQuantizer(hadamard=bad)
    with pytest.raises(ValueError):
        ops.mx_encode_both(x, torch.float8_e4m3fn, hadamard=0)
    with pytest.raises(ValueError):
        ops.mx_encode(torch.zeros(2, 48), torch.float8_e4m3fn, hadamard=0)      # blocks are never short
    with pytest.raises(ValueError):
        ops.mx_quantize_t(torch.zeros(48, 64), torch.float8_e4m3fn, hadamard=0)
    with pytest.raises(ValueError):
        ops.hadamard32(x, None)
