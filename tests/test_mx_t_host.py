"""CPU-only checks of the MX lane with the blocks along dim 0 (csrc/fp8q_mx_t.hip): the header and the ctypes table name the
seven entries, the launch rule (fp8q_mxt_route, host arithmetic) sends shapes where the contract says, argument errors are
told at the C ABI before any launch and in Python before the device check, and MXQuantizer takes block_axis.

The C entries are fp8q_mxt_*: tests/test_mx_host.py and tests/test_mx6_host.py pin the set of fp8q_mx_* entries to the
row-wise lane's six, so the transposed lane has a prefix of its own."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3, E5M2, E2M1 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2
ARITY = {"fp8q_mxt_route": 6, "fp8q_mxt_encode_f32": 8, "fp8q_mxt_encode_h16": 9, "fp8q_mxt_encode_both_f32": 10,
         "fp8q_mxt_encode_both_h16": 11, "fp8q_mxt_quantize_f32": 7, "fp8q_mxt_quantize_h16": 9}
FLOOR, CEIL, F32, F16, BF16 = 0, 1, 0, 1, 2


def test_header_declares_the_entries_and_keeps_the_version():
    text = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    for name, n in ARITY.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == n, name
    assert re.search(r"typedef struct fp8q_mxt_route_info \{[^}]*\bkernel;[^}]*\btile_rows;[^}]*\btile_cols;[^}]*\} fp8q_mxt_route_info;",
                     text)
    assert re.search(r"^#define FP8Q_VERSION 601\b", text, re.M)
    import fp8q
    assert fp8q.lib().fp8q_version() == 601


def test_lib_prototypes_match_the_header():
    import fp8q
    from fp8q import _lib, build
    for name, n in ARITY.items():
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        assert hasattr(fp8q.lib(), name)
    assert "fp8q_mx_t.hip" in build.SOURCES and "fp8q_mxq.h" in build.HEADERS
    # one copy of the device arithmetic: the two units take it from the header and define none of it themselves
    for src in ("fp8q_mx.hip", "fp8q_mx_t.hip"):
        code = open(os.path.join(build.CSRC, src)).read()
        assert '#include "fp8q_mxq.h"' in code
        for fn in ("scale_code(", "scale_inv(", "scale_value(", "mx_q(", "fp4_code(", "fp6_code(", "mx_code4(", "mx_value4(",
                   "umax4(", "umax_xor("):
            assert not re.search(r"^__device__ __forceinline__ \w+ %s" % re.escape(fn), code, re.M), (src, fn)
        assert "struct MxFmt" not in code


def test_route():
    from fp8q import ops
    r = ops.mx_t_route(64, 128, E4M3, torch.float32)
    assert r["kernel"] == "tile"
    assert r["tile_rows"] > 0 and r["tile_rows"] % 32 == 0 and r["tile_cols"] > 0 and r["tile_cols"] % 4 == 0
    assert not r["nontemporal"] and r["code_store_bytes"] == 16
    assert ops.mx_t_route(64, 33, E4M3, torch.float32)["kernel"] == "general"
    assert ops.mx_t_route(64, 128, E4M3, torch.float32, aligned16=False)["kernel"] == "general"
    for dt in (torch.float16, torch.bfloat16):
        assert ops.mx_t_route(64, 36, E4M3, dt)["kernel"] == "general"            # K % 8 != 0
        assert ops.mx_t_route(64, 40, E4M3, dt)["kernel"] == "tile"
    assert ops.mx_t_route(64, 36, E4M3, torch.float32)["kernel"] == "tile"        # K % 4 == 0
    g = ops.mx_t_route(7, 3, "e3m2", torch.float32)
    assert g["kernel"] == "general" and g["tile_rows"] % 32 == 0 and g["tile_cols"] % 4 == 0 and g["tile_rows"] > 0
    # the width of the transposed code stores follows the bytes of a codes_t row
    assert ops.mx_t_route(36, 64, E4M3, torch.float32)["code_store_bytes"] == 4
    assert ops.mx_t_route(31, 64, E5M2, torch.float32)["code_store_bytes"] == 1
    assert ops.mx_t_route(32, 64, E2M1, torch.float32)["code_store_bytes"] == 16
    assert ops.mx_t_route(40, 64, E2M1, torch.float32)["code_store_bytes"] == 4
    assert ops.mx_t_route(64, 64, "e2m3", torch.float32)["code_store_bytes"] == 16
    assert ops.mx_t_route(32, 64, "e2m3", torch.float32)["code_store_bytes"] == 4
    # nontemporal from 64 MiB of float32-sized elements, the lane's rule
    assert ops.mx_t_route(4128, 4100, E4M3, torch.float32)["nontemporal"]
    assert ops.mx_t_route(4128, 4100, E4M3, torch.float32)["kernel"] == "tile"
    assert not ops.mx_t_route(4096, 4095, E4M3, torch.float32)["nontemporal"]
    with pytest.raises(ops.Fp8qError):
        ops.mx_t_route(64, 128, torch.float16, torch.float32)
    with pytest.raises(ops.Fp8qError):
        ops.mx_t_route(0, 128, E4M3, torch.float32)
    with pytest.raises(ops.Fp8qError):
        ops.mx_t_route(64, 128, E4M3, torch.float64)


def test_c_abi_argument_errors_come_before_any_launch():
    import fp8q
    L = fp8q.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63             # never dereferenced: every call below is refused by the checks
    enc, ench = L.fp8q_mxt_encode_f32, L.fp8q_mxt_encode_h16
    both, bothh = L.fp8q_mxt_encode_both_f32, L.fp8q_mxt_encode_both_h16
    qnt, qnth = L.fp8q_mxt_quantize_f32, L.fp8q_mxt_quantize_h16
    # null pointers, empty shapes
    assert enc(None, p, p, 4, 32, 0, FLOOR, None) == -1
    assert enc(p, None, p, 4, 32, 0, FLOOR, None) == -1
    assert ench(p, p, None, BF16, 4, 32, 0, FLOOR, None) == -1
    for i in range(5):
        a = [p] * 5
        a[i] = None
        assert both(*a, 4, 32, 0, FLOOR, None) == -1
        assert bothh(*a, F16, 4, 32, 0, FLOOR, None) == -1
    assert qnt(None, p, 4, 32, 0, FLOOR, None) == -1 and qnt(p, None, 4, 32, 0, FLOOR, None) == -1
    assert qnth(p, None, F16, F16, 4, 32, 0, FLOOR, None) == -1
    for R, K in ((0, 32), (4, 0), (-1, 32)):
        assert enc(p, p, p, R, K, 0, FLOOR, None) == -1
        assert both(p, p, p, p, p, R, K, 0, FLOOR, None) == -1
        assert qnt(p, p, R, K, 0, CEIL, None) == -1
    # unknown formats (3 stays unassigned) are unsupported, an unknown rounding invalid
    for bad in (3, 6, -1):
        assert enc(p, p, p, 4, 32, bad, FLOOR, None) == -2
        assert bothh(p, p, p, p, p, BF16, 4, 32, bad, FLOOR, None) == -2
        assert qnt(p, p, 4, 32, bad, FLOOR, None) == -2
    assert enc(p, p, p, 4, 32, 0, 2, None) == -1 and both(p, p, p, p, p, 4, 32, 0, 2, None) == -1
    assert qnth(p, p, BF16, BF16, 4, 32, 0, -1, None) == -1
    # what packs along R (and, for encode_both, along K) must come out in whole bytes
    assert enc(p, p, p, 5, 32, 2, FLOOR, None) == -1 and ench(p, p, p, F16, 5, 32, 2, FLOOR, None) == -1
    assert both(p, p, p, p, p, 5, 32, 2, FLOOR, None) == -1 and both(p, p, p, p, p, 4, 33, 2, FLOOR, None) == -1
    for f in (4, 5):
        for n in (1, 2, 3, 6, 34):
            assert enc(p, p, p, n, 32, f, FLOOR, None) == -1
            assert both(p, p, p, p, p, n, 32, f, CEIL, None) == -1 and both(p, p, p, p, p, 32, n, f, CEIL, None) == -1
    # a misaligned value pointer; foreign types
    assert enc(p + 2, p, p, 4, 32, 0, FLOOR, None) == -1 and ench(p + 1, p, p, F16, 4, 32, 0, FLOOR, None) == -1
    assert qnt(p, p + 2, 4, 32, 0, FLOOR, None) == -1 and qnth(p + 1, p, F16, F16, 4, 32, 0, FLOOR, None) == -1
    assert ench(p, p, p, F32, 4, 32, 0, FLOOR, None) == -1 and bothh(p, p, p, p, p, 7, 4, 32, 0, FLOOR, None) == -1
    assert qnth(p, p, F16, BF16, 4, 32, 0, FLOOR, None) == -1
    # sizes whose element count or grid overflows
    big = 1 << 62
    assert enc(p, p, p, big, 4, 0, FLOOR, None) == -1 and qnt(p, p, 4, big, 0, FLOOR, None) == -1
    assert both(p, p, p, p, p, 1 << 40, 1 << 40, 0, FLOOR, None) == -1
    assert enc(p, p, p, 1 << 36, 1 << 20, 0, FLOOR, None) == -1                   # 2^28 x 2^14 tiles


@pytest.mark.parametrize("fmt", [E4M3, E2M1, "e2m3", "e3m2"], ids=["e4m3fn", "e2m1", "e2m3", "e3m2"])
def test_ops_geometry_errors_need_no_gpu(fmt):
    from fp8q import ops
    for x in (torch.randn(64), torch.randn(2, 32, 32)):
        with pytest.raises(ops.Fp8qError, match="reshape"):
            ops.mx_encode_t(x, fmt)
        with pytest.raises(ops.Fp8qError, match="reshape"):
            ops.mx_encode_both(x, fmt)
        with pytest.raises(ops.Fp8qError, match="reshape"):
            ops.mx_quantize_t(x, fmt)
    if fmt == E2M1:
        with pytest.raises(ops.Fp8qError, match="even"):
            ops.mx_encode_t(torch.randn(33, 32), fmt)
        with pytest.raises(ops.Fp8qError, match="even"):
            ops.mx_encode_both(torch.randn(33, 32), fmt)
        with pytest.raises(ops.Fp8qError, match="even"):
            ops.mx_encode_both(torch.randn(32, 33), fmt)
    if fmt in ("e2m3", "e3m2"):
        for R in (33, 34, 35):
            with pytest.raises(ops.Fp8qError, match="multiple of 4"):
                ops.mx_encode_t(torch.randn(R, 32), fmt)
            with pytest.raises(ops.Fp8qError, match="multiple of 4"):
                ops.mx_encode_both(torch.randn(32, R), fmt)
    for bad in (torch.float16, "e4m3", 3):
        with pytest.raises(ops.Fp8qError, match="fmt"):
            ops.mx_encode_t(torch.randn(32, 32), bad)
        with pytest.raises(ops.Fp8qError, match="fmt"):
            ops.mx_quantize_t(torch.randn(32, 32), bad)
    with pytest.raises(ops.Fp8qError, match="rounding"):
        ops.mx_encode_t(torch.randn(32, 32), fmt, rounding="nearest")
    with pytest.raises(ops.Fp8qError, match="rounding"):
        ops.mx_encode_both(torch.randn(32, 32), fmt, rounding="up")
    with pytest.raises(ops.Fp8qError, match="rounding"):
        ops.mx_quantize_t(torch.randn(32, 32), fmt, rounding=None)
    # a well-formed call on a CPU tensor gets as far as the device check: there is no CPU path
    for call in (ops.mx_encode_t, ops.mx_encode_both, ops.mx_quantize_t):
        with pytest.raises(ops.Fp8qError, match="CUDA"):
            call(torch.randn(32, 32), fmt)
    # quantize_t packs nothing: an odd R passes the geometry check for every format
    with pytest.raises(ops.Fp8qError, match="CUDA"):
        ops.mx_quantize_t(torch.randn(33, 31), fmt)


def test_quantizer_takes_block_axis():
    from quantization.mx import MXQuantizer
    for bad in (0, 2, 1, -3, None, "rows", True):
        with pytest.raises(ValueError, match="block_axis"):
            MXQuantizer(block_axis=bad)
    q = MXQuantizer(fmt=E5M2, rounding="ceil")
    assert q.block_axis == -1
    legacy = f"fmt=E5M2, rounding=ceil, flatten_rows=False"
    assert legacy in q.extra_repr() and q.extra_repr().endswith("block_axis=-1")
    assert MXQuantizer(block_axis=-1).extra_repr().endswith("block_axis=-1")
    qt = MXQuantizer(fmt="e2m3", block_axis=-2, flatten_rows=True)
    assert qt.block_axis == -2 and qt.extra_repr().endswith("block_axis=-2") and "E2M3" in qt.extra_repr()
    # geometry is told before the device check: not a matrix; a dim 0 that the format's packing cannot take
    from fp8q import ops
    with pytest.raises(ops.Fp8qError, match="reshape"):
        MXQuantizer(block_axis=-2)(torch.randn(8, 4, 3, 3))
    with pytest.raises(ops.Fp8qError, match="multiple of 4"):
        qt(torch.randn(6, 4, 3, 3))
    with pytest.raises(ops.Fp8qError, match="multiple of 4"):
        qt.encode(torch.randn(6, 4, 3, 3))
    with pytest.raises(ops.Fp8qError, match="CUDA"):
        qt(torch.randn(8, 4, 3, 3))
