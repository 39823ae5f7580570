"""CPU-only checks of the 6-bit microscaling formats (E2M3 / E3M2, csrc/fp8q_mx.hip): the oracle of tests/mx6_oracle.py on
values whose codes can be written down by hand, the C ABI's argument checks for the two new format ids (reported before any
launch, so they need no GPU), and the Python surface -- the string format names, the geometry errors, MXQuantizer."""
import ctypes
import os
import re

import pytest
import torch

import mx6_oracle as mx6
from mx6_oracle import E2M3, E3M2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MX = ("fp8q_mx_encode_f32", "fp8q_mx_encode_h16", "fp8q_mx_decode_f32", "fp8q_mx_decode_h16", "fp8q_mx_quantize_f32",
      "fp8q_mx_quantize_h16")
ID = {E2M3: 4, E3M2: 5}
FLOOR, CEIL = 0, 1
F16, BF16 = 1, 2

# the 32 magnitudes of each format, code by code
E2M3_VALUES = [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875,
               1.0, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
               2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75,
               4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5]
E3M2_VALUES = [0.0, 0.0625, 0.125, 0.1875, 0.25, 0.3125, 0.375, 0.4375,
               0.5, 0.625, 0.75, 0.875, 1.0, 1.25, 1.5, 1.75,
               2.0, 2.5, 3.0, 3.5, 4.0, 5.0, 6.0, 7.0,
               8.0, 10.0, 12.0, 14.0, 16.0, 20.0, 24.0, 28.0]
VALUES = {E2M3: E2M3_VALUES, E3M2: E3M2_VALUES}


def _block(vals):
    x = torch.zeros(1, 32)
    x[0, :len(vals)] = torch.tensor(vals)
    return x


def test_oracle_packs_1_2_3_4_into_08_44_61():
    c, s, v = mx6.oracle(_block([1.0, 2.0, 3.0, 4.0]), E2M3, "floor")
    assert s.tolist() == [[127]] and tuple(c.shape) == (1, 24)
    assert c[0, :3].tolist() == [0x08, 0x44, 0x61] and c[0, 3:].tolist() == [0] * 21
    assert mx6.unpack(c)[0, :5].tolist() == [8, 16, 20, 24, 0]
    assert v[0, :4].tolist() == [1.0, 2.0, 3.0, 4.0]
    # the same four under E3M2: the largest, 4 = 2^2, sits two binades under emax, so X = 2^-2 and q = 4, 8, 12, 16
    c, s, v = mx6.oracle(_block([1.0, 2.0, 3.0, 4.0]), E3M2, "floor")
    assert s.tolist() == [[125]] and mx6.unpack(c)[0, :4].tolist() == [20, 24, 26, 28]
    assert v[0, :4].tolist() == [1.0, 2.0, 3.0, 4.0]
    c, s, v = mx6.oracle(_block([16.0, 1.0, 2.0, 3.0, 4.0]), E3M2, "floor")
    assert s.tolist() == [[127]] and mx6.unpack(c)[0, :5].tolist() == [28, 12, 16, 18, 20]


@pytest.mark.parametrize("fmt,anchor,cases", [
    # (x, code, value): midpoints of neighbouring codes go to the even one; the first element pins the scale to 1
    (E2M3, 4.0, [(0.0625, 0, 0.0), (0.1875, 2, 0.25), (0.9375, 8, 1.0), (1.0625, 8, 1.0), (1.1875, 10, 1.25),
                 (2.125, 16, 2.0), (3.875, 24, 4.0), (-0.0625, 0x20, -0.0), (-1.1875, 0x2A, -1.25), (7.25, 30, 7.0),
                 (-0.0, 0x20, -0.0), (0.0, 0, 0.0), (7.75, 31, 7.5), (-7.9, 0x3F, -7.5), (1e-30, 0, 0.0)]),
    (E3M2, 16.0, [(0.03125, 0, 0.0), (0.09375, 2, 0.125), (0.21875, 4, 0.25), (1.125, 12, 1.0), (1.375, 14, 1.5),
                  (1.875, 16, 2.0), (15.0, 28, 16.0), (-0.09375, 0x22, -0.125), (-0.0, 0x20, -0.0), (26.0, 30, 24.0),
                  (30.0, 31, 28.0), (-31.0, 0x3F, -28.0), (-1e-30, 0x20, -0.0)]),
], ids=[E2M3, E3M2])
def test_oracle_ties_signed_zero_and_saturation(fmt, anchor, cases):
    c, s, v = mx6.oracle(_block([anchor] + [x for x, _, _ in cases]), fmt, "floor")
    assert s.tolist() == [[127]]
    n = len(cases)
    assert mx6.unpack(c)[0, 1:n + 1].tolist() == [code for _, code, _ in cases]
    want = torch.tensor([val for _, _, val in cases])
    assert torch.equal(v[0, 1:n + 1].view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("E", [0, 3, -20])
def test_oracle_floor_saturates_where_ceil_bumps(E):
    """E2M3: an amax of 7.75 * 2^E has the mantissa field 0x780000 > 0x700000; E3M2: 30 * 2^E has 0x700000 > 0x600000"""
    for fmt, amax, fmax, emax in ((E2M3, 7.75, 7.5, 2), (E3M2, 30.0, 28.0, 4)):
        x = _block([amax * 2.0 ** E, -fmax * 2.0 ** E])
        c, s, v = mx6.oracle(x, fmt, "floor")
        assert s.tolist() == [[127 + E]] and mx6.unpack(c)[0, :2].tolist() == [31, 63]
        assert v[0, :2].tolist() == [fmax * 2.0 ** E, -fmax * 2.0 ** E]                 # saturated
        c, s, v = mx6.oracle(x, fmt, "ceil")
        assert s.tolist() == [[128 + E]]
        # amax / 2 is the midpoint under the power of two 2^emax: the tie goes to the even code, whose mantissa is 0
        top = (emax + mx6.BIAS[fmt]) << mx6.MBITS[fmt]
        assert mx6.unpack(c)[0, :2].tolist() == [top, (top - 1) | 32]
        assert v[0, :2].tolist() == [2.0 ** emax * 2.0 ** (E + 1), -fmax * 2.0 ** E]
        # at man_fmax itself nothing bumps
        assert mx6.oracle(_block([fmax * 2.0 ** E]), fmt, "ceil")[1].tolist() == [[127 + E]]


@pytest.mark.parametrize("fmt", mx6.FMTS)
def test_oracle_decodes_all_64_codes(fmt):
    c = torch.arange(64)
    table = torch.tensor(VALUES[fmt] + [-t for t in VALUES[fmt]])
    assert torch.equal(mx6.element_value(c, fmt).view(torch.int32), table.view(torch.int32))
    assert max(VALUES[fmt]) == mx6.FMAX[fmt]
    # packed, under a scale of 2 and under the NaN scale; and every value encodes back to its own code
    b = mx6.pack(c.view(1, 64))
    assert tuple(b.shape) == (1, 48) and torch.equal(mx6.unpack(b), c.view(1, 64))
    v = mx6.decode(b, torch.tensor([[128, 255]], dtype=torch.uint8), fmt)
    assert torch.equal(v[0, :32], 2 * table[:32]) and torch.isnan(v[0, 32:]).all()
    codes, mag = mx6.element_codes(table, fmt)
    assert torch.equal(codes, c) and torch.equal(mag, table.abs())
    # a NaN or an infinity anywhere: the block's scale is 0xFF, its codes are 0, its values NaN
    for bad in (float("nan"), float("inf"), -float("inf")):
        cc, s, vv = mx6.oracle(_block([1.0, bad, -2.0]), fmt, "floor")
        assert s.tolist() == [[255]] and not cc.any() and torch.isnan(vv).all()


def test_header_defines_the_two_ids_and_keeps_the_version():
    text = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    defs = dict(re.findall(r"^#define (FP8Q_MX_\w+) (-?\d+)$", text, re.M))
    assert defs == {"FP8Q_MX_E4M3FN": "0", "FP8Q_MX_E5M2": "1", "FP8Q_MX_E2M1": "2", "FP8Q_MX_E2M3": "4", "FP8Q_MX_E3M2": "5",
                    "FP8Q_MX_FLOOR": "0", "FP8Q_MX_CEIL": "1"}
    assert re.search(r"^#define FP8Q_VERSION 601\b", text, re.M)
    import fp8q
    assert fp8q.lib().fp8q_version() == 601
    assert {n for n in fp8q._lib.SIGNATURES if n.startswith("fp8q_mx_")} == set(MX)         # no new entry points


@pytest.mark.parametrize("fmt", mx6.FMTS)
def test_c_abi_argument_errors_come_before_any_launch(fmt):
    import fp8q
    L = fp8q.lib()
    f = ID[fmt]
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63             # never dereferenced: every call below is refused by the checks
    enc, ench = L.fp8q_mx_encode_f32, L.fp8q_mx_encode_h16
    dec, dech = L.fp8q_mx_decode_f32, L.fp8q_mx_decode_h16
    qnt, qnth = L.fp8q_mx_quantize_f32, L.fp8q_mx_quantize_h16
    # a row length that is no multiple of 4, on all six entries
    for K in (1, 2, 3, 30, 33, 34, 35, 4098):
        assert enc(p, p, p, 4, K, f, FLOOR, None) == -1, K
        assert ench(p, p, p, BF16, 4, K, f, CEIL, None) == -1, K
        assert dec(p, p, p, 4, K, f, None) == -1, K
        assert dech(p, p, p, F16, 4, K, f, None) == -1, K
        assert qnt(p, p, 4, K, f, CEIL, None) == -1, K
        assert qnth(p, p, F16, F16, 4, K, f, FLOOR, None) == -1, K
    # the ids around the new ones stay unsupported: 3 is unassigned
    for bad in (3, 6, 7, -1):
        assert enc(p, p, p, 4, 32, bad, FLOOR, None) == -2
        assert ench(p, p, p, F16, 4, 32, bad, FLOOR, None) == -2
        assert dec(p, p, p, 4, 32, bad, None) == -2
        assert dech(p, p, p, BF16, 4, 32, bad, None) == -2
        assert qnt(p, p, 4, 32, bad, FLOOR, None) == -2
        assert qnth(p, p, BF16, BF16, 4, 32, bad, FLOOR, None) == -2
    # null pointers
    assert enc(None, p, p, 4, 32, f, FLOOR, None) == -1
    assert enc(p, None, p, 4, 32, f, FLOOR, None) == -1
    assert enc(p, p, None, 4, 32, f, FLOOR, None) == -1
    assert ench(p, p, None, F16, 4, 32, f, FLOOR, None) == -1
    assert dec(None, p, p, 4, 32, f, None) == -1
    assert dec(p, None, p, 4, 32, f, None) == -1
    assert dec(p, p, None, 4, 32, f, None) == -1
    assert dech(p, None, p, BF16, 4, 32, f, None) == -1
    assert qnt(None, p, 4, 32, f, CEIL, None) == -1
    assert qnt(p, None, 4, 32, f, CEIL, None) == -1
    assert qnth(None, p, F16, F16, 4, 32, f, CEIL, None) == -1
    # empty tensors, an unknown rounding, foreign types
    assert enc(p, p, p, 0, 32, f, FLOOR, None) == -1
    assert dec(p, p, p, 4, 0, f, None) == -1
    assert qnt(p, p, 4, 32, f, 2, None) == -1
    assert ench(p, p, p, 0, 4, 32, f, FLOOR, None) == -1
    assert qnth(p, p, F16, BF16, 4, 32, f, FLOOR, None) == -1
    # a misaligned value pointer (codes and scale bytes may lie anywhere)
    assert enc(p + 2, p, p, 4, 32, f, FLOOR, None) == -1
    assert ench(p + 1, p, p, F16, 4, 32, f, FLOOR, None) == -1
    assert dec(p, p, p + 2, 4, 32, f, None) == -1
    assert dech(p, p, p + 1, BF16, 4, 32, f, None) == -1
    assert qnt(p, p + 1, 4, 32, f, FLOOR, None) == -1
    assert qnth(p + 1, p, F16, F16, 4, 32, f, FLOOR, None) == -1


@pytest.mark.parametrize("fmt", mx6.FMTS)
def test_ops_geometry_errors_need_no_gpu(fmt):
    from fp8q import ops
    assert (ops.MX_E2M3, ops.MX_E3M2) == ("e2m3", "e3m2") and ops._MX_FMT[fmt] == ID[fmt] and 3 not in ops._MX_FMT.values()
    for K in (2, 31, 33, 147):
        with pytest.raises(ops.Fp8qError, match="multiple of 4"):
            ops.mx_encode(torch.randn(4, K), fmt)
        with pytest.raises(ops.Fp8qError, match="multiple of 4"):
            ops.mx_quantize(torch.randn(4, K).bfloat16(), fmt, rounding="ceil")
    scales = torch.full((4, 2), 127, dtype=torch.uint8)
    for n in (47, 49, 1):
        with pytest.raises(ops.Fp8qError, match="multiple of 3"):
            ops.mx_decode(torch.zeros(4, n, dtype=torch.uint8), scales, fmt=fmt)
    with pytest.raises(ops.Fp8qError, match="carry no format"):
        ops.mx_decode(torch.zeros(4, 48, dtype=torch.uint8), scales)
    # a sound call on CPU tensors gets as far as the refusal of the device: there is no CPU path and no fallback
    with pytest.raises(ops.Fp8qError, match="CUDA"):
        ops.mx_encode(torch.randn(4, 64), fmt)
    with pytest.raises(ops.Fp8qError, match="CUDA"):
        ops.mx_quantize(torch.randn(4, 36), fmt)
    with pytest.raises(ops.Fp8qError, match="CUDA"):
        ops.mx_decode(torch.zeros(4, 48, dtype=torch.uint8), scales, fmt=fmt)
    # the message about formats names the new ones and begins as it did
    for bad in ("e2m1", "E2M3", 4, None, torch.float16):
        with pytest.raises(ops.Fp8qError, match=r"^fmt must be .*'e2m3' or 'e3m2'"):
            ops.mx_encode(torch.randn(4, 64), bad)


def test_quantizer_takes_the_fp6_formats():
    from quantization.mx import MXQuantizer
    for fmt, name in ((E2M3, "E2M3"), (E3M2, "E3M2")):
        q = MXQuantizer(fmt=fmt)
        assert q.n_bits == 6 and q.fmt == fmt and q.rounding == "floor" and not q.keep_dtype and not q.flatten_rows
        assert MXQuantizer(n_bits=6, fmt=fmt, rounding="ceil", keep_dtype=True, flatten_rows=True).n_bits == 6
        assert name in q.extra_repr()
        for n in (8, 4):
            with pytest.raises(ValueError, match="6 bits"):
                MXQuantizer(n_bits=n, fmt=fmt)
        w = torch.zeros(8, 4, 3, 3)
        assert tuple(MXQuantizer(fmt=fmt, flatten_rows=True)._rows(w).shape) == (8, 36)
    for bad in ("e2m1", "fp6", 6):
        with pytest.raises(ValueError, match="fmt must be"):
            MXQuantizer(fmt=bad)
    with pytest.raises(ValueError):
        MXQuantizer(n_bits=6)                         # the default format has 8


def test_a_conv_weight_with_147_element_rows_raises_and_is_not_padded():
    from fp8q import ops
    from quantization.mx import MXQuantizer
    q = MXQuantizer(fmt=E3M2, flatten_rows=True)
    w = torch.randn(64, 3, 7, 7)
    with pytest.raises(ops.Fp8qError, match="multiple of 4, got 147"):
        q(w)
    with pytest.raises(ops.Fp8qError, match="multiple of 4, got 147"):
        q.encode(w)
