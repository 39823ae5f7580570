"""CPU-only checks of the transposed operands of the tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block_t.hip): the library
exports exactly the five fp8q_ocpbt_* entries and reports every argument error before any launch, fp8q_ocpbt_route answers
without a GPU for every shape the GPU tests use, the Python wrappers refuse CPU tensors, tensors that are no matrix, the tile
(128, 1), bad formats and wrong output buffers (there is no fallback), and OCPBlockFP8Quantizer has encode_t / encode_both.

The C entries are fp8q_ocpbt_*: tests/test_ocpb_host.py pins the set of fp8q_ocpb_* entries to the lane's seven."""
import ctypes
import os
import re

import pytest
import torch

import ocpb_oracle as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"fp8q_ocpbt_route": 7, "fp8q_ocpbt_encode_f32": 10, "fp8q_ocpbt_encode_h16": 11, "fp8q_ocpbt_encode_both_f32": 12,
         "fp8q_ocpbt_encode_both_h16": 13}
E4M3FN, E5M2 = 0, 1
F32, F16, BF16 = 0, 1, 2
PANEL, PLAIN = 0, 1
FMTS = (torch.float8_e4m3fn, torch.float8_e5m2)
ROW, COL, FULL = (1, 128), (128, 1), (128, 128)
# shape -> (kernel, bytes per store of transposed codes) of an aligned tensor: the table of the GPU tests
SHAPES = {(1, 1): ("plain", 1), (127, 5): ("plain", 1), (129, 131): ("plain", 1), (128, 128): ("panel", 16),
          (256, 384): ("panel", 16), (144, 260): ("panel", 16), (132, 132): ("panel", 4), (130, 260): ("panel", 1),
          (5, 132): ("panel", 1)}


def test_library_exports_exactly_the_five_symbols():
    import fp8q
    from fp8q import _lib, build
    lib = ctypes.CDLL(fp8q.so_path())
    for n, arity in ARITY.items():
        assert hasattr(lib, n), n
        res, args = _lib.SIGNATURES[n]
        assert res is ctypes.c_int and len(args) == arity, n
    assert {n for n in _lib.SIGNATURES if n.startswith("fp8q_ocpbt_")} == set(ARITY)
    assert fp8q.lib().fp8q_version() == 601           # the entries are additive
    assert "fp8q_ocp_block_t.hip" in build.SOURCES and "fp8q_ocpq.h" in build.HEADERS and "fp8q_mxq.h" in build.HEADERS
    text = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    for n, arity in ARITY.items():
        m = re.search(r"^int %s\(([^;]*)\);" % n, text, re.M)
        assert m and len(m.group(1).split(",")) == arity, n
    assert re.search(r"typedef struct fp8q_ocpbt_route_info \{[^}]*\bkernel;[^}]*\bcode_store_bytes;[^}]*\bnontemporal;[^}]*\} "
                     r"fp8q_ocpbt_route_info;", text)
    assert re.search(r"^#define FP8Q_OCPBT_PANEL 0$", text, re.M) and re.search(r"^#define FP8Q_OCPBT_PLAIN 1$", text, re.M)
    # one copy of the device arithmetic: the unit takes it from the two headers and defines none of it itself
    code = open(os.path.join(build.CSRC, "fp8q_ocp_block_t.hip")).read()
    assert '#include "fp8q_ocpq.h"' in code and '#include "fp8q_mxq.h"' in code
    for fn in ("ocp_scale_pair(", "code_exact(", "clamp_end(", "code4(", "code1(", "abs_bits(", "umax4(", "umax_xor("):
        assert not re.search(r"^__device__ __forceinline__ \w+ %s" % re.escape(fn), code, re.M), fn
    assert "struct OcpFmt" not in code


def test_argument_errors_come_before_any_launch():
    import fp8q
    L = fp8q.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63             # never dereferenced: every call below is refused by the checks
    enc, ench = L.fp8q_ocpbt_encode_f32, L.fp8q_ocpbt_encode_h16
    both, bothh = L.fp8q_ocpbt_encode_both_f32, L.fp8q_ocpbt_encode_both_h16
    # null pointers
    for i in range(3):
        a = [p] * 3
        a[i] = None
        assert enc(*a, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
        assert ench(*a, F16, 4, 128, 128, 128, E5M2, 1e-8, None) == -1
    for i in range(5):
        a = [p] * 5
        a[i] = None
        assert both(*a, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
        assert bothh(*a, BF16, 4, 128, 128, 128, E4M3FN, 1e-8, None) == -1
    # empty tensors, an element count beyond int64
    for R, K in ((0, 128), (4, 0), (-1, 128), (4, -1), (1 << 62, 4), (4, 1 << 62)):
        assert enc(p, p, p, R, K, 1, 128, E4M3FN, 1e-8, None) == -1, (R, K)
        assert ench(p, p, p, BF16, R, K, 128, 128, E4M3FN, 1e-8, None) == -1, (R, K)
        assert both(p, p, p, p, p, R, K, 128, 128, E4M3FN, 1e-8, None) == -1, (R, K)
        assert bothh(p, p, p, p, p, F16, R, K, 1, 128, E5M2, 1e-8, None) == -1, (R, K)
    # a value pointer off its element's alignment, scales off 4 bytes (codes may lie anywhere)
    assert enc(p + 2, p, p, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert enc(p, p, p + 2, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert ench(p + 1, p, p, F16, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert ench(p, p, p + 1, BF16, 4, 128, 128, 128, E4M3FN, 1e-8, None) == -1
    assert both(p + 1, p, p, p, p, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert both(p, p, p + 2, p, p, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert both(p, p, p, p, p + 2, 4, 128, 128, 128, E4M3FN, 1e-8, None) == -1
    assert bothh(p + 1, p, p, p, p, F16, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert bothh(p, p, p + 3, p, p, BF16, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert bothh(p, p, p, p, p + 1, BF16, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    # types: a half entry takes half types
    for bad in (F32, 3, -1):
        assert ench(p, p, p, bad, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
        assert bothh(p, p, p, p, p, bad, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    # any other format; any other tile, (128, 1) among them
    for fmt in (2, -1, 7):
        assert enc(p, p, p, 4, 128, 1, 128, fmt, 1e-8, None) == -2
        assert ench(p, p, p, F16, 4, 128, 128, 128, fmt, 1e-8, None) == -2
        assert both(p, p, p, p, p, 4, 128, 1, 128, fmt, 1e-8, None) == -2
        assert bothh(p, p, p, p, p, BF16, 4, 128, 128, 128, fmt, 1e-8, None) == -2
    info = fp8q._lib.OcpbtRouteInfo()
    for tr, tk in ((128, 1), (1, 1), (1, 64), (64, 64), (128, 64), (1, 256), (0, 128), (128, 0), (-1, 128), (32, 1), (128, 2)):
        assert enc(p, p, p, 4, 128, tr, tk, E4M3FN, 1e-8, None) == -2, (tr, tk)
        assert ench(p, p, p, BF16, 4, 128, tr, tk, E5M2, 1e-8, None) == -2, (tr, tk)
        assert both(p, p, p, p, p, 4, 128, tr, tk, E4M3FN, 1e-8, None) == -2, (tr, tk)
        assert bothh(p, p, p, p, p, F16, 4, 128, tr, tk, E5M2, 1e-8, None) == -2, (tr, tk)
        assert L.fp8q_ocpbt_route(4, 128, tr, tk, F32, 1, ctypes.byref(info)) == -2, (tr, tk)
    # a grid beyond INT32_MAX: 2^33 panels; 2^40 column tiles on the plain route (K % 4 != 0)
    assert enc(p, p, p, 1 << 40, 4, 128, 128, E4M3FN, 1e-8, None) == -1
    assert both(p, p, p, p, p, 4, 1 << 40, 1, 128, E4M3FN, 1e-8, None) == -1
    assert enc(p, p, p, 4, (1 << 40) + 1, 1, 128, E4M3FN, 1e-8, None) == -1
    assert bothh(p, p, p, p, p, F16, (1 << 40) + 1, 5, 1, 128, E4M3FN, 1e-8, None) == -1


def test_route_answers_without_a_gpu():
    import fp8q
    from fp8q import ops
    route = fp8q.lib().fp8q_ocpbt_route
    info = fp8q._lib.OcpbtRouteInfo()
    for xt in (F32, F16, BF16):
        for tr, tk in (ROW, FULL):
            for (R, K), (kernel, width) in SHAPES.items():
                assert route(R, K, tr, tk, xt, 1, ctypes.byref(info)) == 0
                assert (info.kernel, info.code_store_bytes, info.nontemporal) == (PANEL if kernel == "panel" else PLAIN, width, 0)
                assert route(R, K, tr, tk, xt, 0, ctypes.byref(info)) == 0
                assert (info.kernel, info.code_store_bytes, info.nontemporal) == (PLAIN, 1, 0), (R, K)
    assert route(4, 128, 1, 128, F32, 1, None) == -1
    assert route(0, 128, 1, 128, F32, 1, ctypes.byref(info)) == -1 and route(4, 0, 1, 128, F32, 1, ctypes.byref(info)) == -1
    assert route(4, 128, 1, 128, 3, 1, ctypes.byref(info)) == -1
    assert route(1 << 62, 4, 1, 128, F32, 1, ctypes.byref(info)) == -1
    assert ops.OCP_BLOCK_T_KERNELS == ("panel", "plain") and ops.OCP_BLOCK_T_TILES == (ROW, FULL)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        for tile in (ROW, [128, 128]):
            for (R, K), (kernel, width) in SHAPES.items():
                assert ops.ocp_block_t_route(R, K, tile, dt) == {"kernel": kernel, "code_store_bytes": width,
                                                                 "nontemporal": False}, (R, K)
                assert ops.ocp_block_t_route(R, K, tile, dt, aligned16=False)["kernel"] == "plain"
    assert {v for v in SHAPES.values()} == {("plain", 1), ("panel", 16), ("panel", 4), ("panel", 1)}
    # nontemporal from 64 MiB of float32-sized elements, the lane's rule, on the panel route only
    big = ops.ocp_block_t_route(4112, 4096, ROW, torch.float32)
    assert big == {"kernel": "panel", "code_store_bytes": 16, "nontemporal": True}
    assert ops.ocp_block_t_route(4112, 4096, FULL, torch.bfloat16)["nontemporal"]
    assert not ops.ocp_block_t_route(4096, 4092, ROW, torch.float32)["nontemporal"]
    assert not ops.ocp_block_t_route(4112, 4097, ROW, torch.float32)["nontemporal"]
    with pytest.raises(ops.Fp8qError, match="no transposed operands"):
        ops.ocp_block_t_route(256, 384, COL, torch.float32)
    with pytest.raises(ops.Fp8qError, match="tile must be"):
        ops.ocp_block_t_route(256, 384, (64, 64), torch.float32)
    with pytest.raises(ops.Fp8qError, match="dtype must be"):
        ops.ocp_block_t_route(256, 384, ROW, torch.float64)
    with pytest.raises(ops.Fp8qError):
        ops.ocp_block_t_route(0, 384, ROW, torch.float32)


@pytest.mark.parametrize("tile", (ROW, FULL))
@pytest.mark.parametrize("fmt", FMTS)
def test_ops_raise_on_cpu_tensors(fmt, tile):
    from fp8q import ops
    for x in (torch.randn(4, 256), torch.randn(130, 260).bfloat16(), torch.randn(5, 3).half()):
        with pytest.raises(ops.Fp8qError, match="no CPU path"):
            ops.ocp_block_encode_t(x, fmt, tile)
        with pytest.raises(ops.Fp8qError, match="no CPU path"):
            ops.ocp_block_encode_both(x, fmt, tile)
    for x in (None, [[1.0]], 1.0):
        with pytest.raises(ops.Fp8qError, match="no CPU path"):
            ops.ocp_block_encode_t(x, fmt, tile)
        with pytest.raises(ops.Fp8qError, match="no CPU path"):
            ops.ocp_block_encode_both(x, fmt, tile)


def test_ops_refuse_other_ranks_tiles_and_formats():
    from fp8q import ops
    fmt = torch.float8_e4m3fn
    x = torch.randn(4, 256)
    for call in (ops.ocp_block_encode_t, ops.ocp_block_encode_both):
        for bad in (torch.randn(256), torch.randn(2, 3, 128), torch.tensor(1.0)):
            for tile in (ROW, FULL):
                with pytest.raises(ops.Fp8qError, match="reshape"):
                    call(bad, fmt, tile)
        with pytest.raises(ops.Fp8qError, match="no transposed operands"):
            call(x, fmt, COL)
        with pytest.raises(ops.Fp8qError, match="no transposed operands"):
            call(x, fmt, [128, 1])
        for tile in ((64, 64), (1, 32), (128,), None, 128, (128, 128, 1), (True, 128)):
            with pytest.raises(ops.Fp8qError, match="tile must be"):
                call(x, fmt, tile)
        for bad in (torch.float16, torch.uint8, torch.float4_e2m1fn_x2, getattr(torch, "float8_e4m3fnuz", torch.int8), "e2m3"):
            with pytest.raises(ops.Fp8qError, match="fmt must be"):
                call(x, bad)
            with pytest.raises(ops.Fp8qError, match="fmt must be"):
                call(x, bad, FULL)
    assert not hasattr(ops, "ocp_block_quantize_t")           # column-tile fake-quantization is ocp_block_quantize(tile=(128, 1))


@pytest.mark.parametrize("tile", (ROW, FULL))
def test_ops_refuse_wrong_output_buffers(tile):
    """told from the buffers' dtype and shape alone, before the device check: each call below would otherwise end at the
    refusal of the CPU tensor x, whose message is another"""
    from fp8q import ops
    fmt = torch.float8_e4m3fn
    R, K = 130, 260
    x = torch.randn(R, K)
    sshape = ob.oracle(torch.zeros(R, K), fmt, tile)[1].shape
    stshape = ob.oracle(torch.zeros(K, R), fmt, tile)[1].shape
    assert sshape == ((R, 3) if tile == ROW else (2, 3)) and stshape == ((K, 2) if tile == ROW else (3, 2))
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    f32 = lambda *s: torch.zeros(*s)
    bad_codes = (u8(R * K + 1), u8(R, K - 1), f32(R, K), torch.zeros(R, K, dtype=torch.float8_e5m2), u8(K, 2 * R)[:, ::2],
                 "codes")
    for b in bad_codes:
        with pytest.raises(ops.Fp8qError, match="out must be"):
            ops.ocp_block_encode_t(x, fmt, tile, out=b)
        with pytest.raises(ops.Fp8qError, match="out must be"):
            ops.ocp_block_encode_both(x, fmt, tile, out=b)
        with pytest.raises(ops.Fp8qError, match="out_t must be"):
            ops.ocp_block_encode_both(x, fmt, tile, out_t=b)

    def bad_scales(shape):
        n = shape[0] * shape[1]
        return (f32(shape[0] + 1, shape[1]), f32(shape[0], shape[1] + 1), f32(n), f32(*shape[::-1]),
                torch.zeros(shape, dtype=torch.float16), torch.zeros(shape, dtype=torch.float64), u8(*shape),
                f32(shape[0], 2 * shape[1])[:, ::2], 1.0)

    for b in bad_scales(stshape):
        with pytest.raises(ops.Fp8qError, match="scales_out must be"):
            ops.ocp_block_encode_t(x, fmt, tile, scales_out=b)
        with pytest.raises(ops.Fp8qError, match="scales_out_t must be"):
            ops.ocp_block_encode_both(x, fmt, tile, scales_out_t=b)
    for b in bad_scales(sshape):
        with pytest.raises(ops.Fp8qError, match="scales_out must be"):
            ops.ocp_block_encode_both(x, fmt, tile, scales_out=b)
    # well-formed buffers get as far as the device check: there is no CPU path
    with pytest.raises(ops.Fp8qError, match="no CPU path"):
        ops.ocp_block_encode_t(x, fmt, tile, out=u8(K, R), scales_out=f32(*stshape))
    with pytest.raises(ops.Fp8qError, match="no CPU path"):
        ops.ocp_block_encode_both(x, fmt, tile, out=u8(R * K), scales_out=f32(*sshape),
                                  out_t=torch.zeros(K, R, dtype=fmt), scales_out_t=f32(*stshape))


def test_quantizer_has_the_transposed_encoders():
    from fp8q import ops
    from quantization.ocp import OCPBlockFP8Quantizer as Q
    for tile in (ROW, FULL):
        q = Q(fmt=torch.float8_e5m2, tile=tile, eps=1e-4, flatten_rows=True)
        assert callable(q.encode_t) and callable(q.encode_both)
        # a well-formed call gets as far as the op's refusal of a CPU tensor; flatten_rows makes a matrix of a conv weight
        for call in (q.encode_t, q.encode_both):
            with pytest.raises(ops.Fp8qError, match="no CPU path"):
                call(torch.randn(8, 3, 3, 3))
            with pytest.raises(ops.Fp8qError, match="no CPU path"):
                call(torch.randn(136, 256, requires_grad=True))
        for call in (Q(tile=tile).encode_t, Q(tile=tile).encode_both):
            with pytest.raises(ops.Fp8qError, match="reshape"):           # without flatten_rows it stays 4-D
                call(torch.randn(8, 3, 3, 3))
    qc = Q(tile=COL)
    for call in (qc.encode_t, qc.encode_both):
        with pytest.raises(ValueError, match="no transposed operands"):
            call(torch.randn(136, 256))
    assert not hasattr(qc, "quantize_t")
