"""CPU-only checks of the tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block.hip): the library exports its seven entry points
and reports every argument error before any launch, fp8q_ocpb_route answers without a GPU, the Python wrappers refuse CPU
tensors, bad tiles, bad formats and wrong scale shapes (there is no fallback), OCPBlockFP8Quantizer follows the quantizer
protocol without being one of the CLI's methods or ever giving its manager's estimator work, and the oracle the GPU tests use
has the properties the contract states."""
import ctypes

import pytest
import torch

import ocpb_oracle as ob

OCPB = ("fp8q_ocpb_route", "fp8q_ocpb_encode_f32", "fp8q_ocpb_encode_h16", "fp8q_ocpb_decode_f32", "fp8q_ocpb_decode_h16",
        "fp8q_ocpb_quantize_f32", "fp8q_ocpb_quantize_h16")
E4M3FN, E5M2 = 0, 1
F32, F16, BF16 = 0, 1, 2
ROWS, PANEL, PLAIN = 0, 1, 2
FMTS = (torch.float8_e4m3fn, torch.float8_e5m2)


def test_library_exports_exactly_the_seven_symbols():
    import fp8q
    from fp8q import build
    lib = ctypes.CDLL(fp8q.so_path())
    for n in OCPB:
        assert hasattr(lib, n), n
        assert n in fp8q._lib.SIGNATURES, n
    assert {n for n in fp8q._lib.SIGNATURES if n.startswith("fp8q_ocpb_")} == set(OCPB)
    assert fp8q.lib().fp8q_version() == 601           # the entries are additive
    assert "fp8q_ocp_block.hip" in build.SOURCES and "fp8q_ocpq.h" in build.HEADERS


def test_argument_errors_come_before_any_launch():
    import fp8q
    L = fp8q.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63             # never dereferenced: every call below is refused by the checks
    enc, ench = L.fp8q_ocpb_encode_f32, L.fp8q_ocpb_encode_h16
    dec, dech = L.fp8q_ocpb_decode_f32, L.fp8q_ocpb_decode_h16
    qnt, qnth = L.fp8q_ocpb_quantize_f32, L.fp8q_ocpb_quantize_h16
    # null pointers
    assert enc(None, p, p, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert enc(p, None, p, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert enc(p, p, None, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert ench(None, p, p, F16, 4, 128, 128, 1, E4M3FN, 1e-8, None) == -1
    assert dec(None, p, p, 4, 128, 128, 128, E5M2, None) == -1
    assert dec(p, None, p, 4, 128, 128, 128, E5M2, None) == -1
    assert dec(p, p, None, 4, 128, 128, 128, E5M2, None) == -1
    assert dech(p, p, None, BF16, 4, 128, 1, 128, E5M2, None) == -1
    assert qnt(None, p, 4, 128, 128, 1, E4M3FN, 1e-8, None) == -1
    assert qnt(p, None, 4, 128, 128, 1, E4M3FN, 1e-8, None) == -1
    assert qnth(p, None, F16, F16, 4, 128, 128, 1, E4M3FN, 1e-8, None) == -1
    # empty tensors
    assert enc(p, p, p, 0, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert enc(p, p, p, 4, 0, 1, 128, E4M3FN, 1e-8, None) == -1
    assert dec(p, p, p, 4, -1, 1, 128, E4M3FN, None) == -1
    assert qnt(p, p, 0, 0, 128, 128, E4M3FN, 1e-8, None) == -1
    # a value pointer off its element's alignment, scales off 4 bytes (codes may lie anywhere)
    assert enc(p + 2, p, p, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert enc(p, p, p + 2, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert ench(p + 1, p, p, F16, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert ench(p, p, p + 1, BF16, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert dec(p, p, p + 2, 4, 128, 128, 1, E4M3FN, None) == -1
    assert dec(p, p + 2, p, 4, 128, 128, 1, E4M3FN, None) == -1
    assert dech(p, p, p + 1, BF16, 4, 128, 128, 1, E4M3FN, None) == -1
    assert qnt(p, p + 1, 4, 128, 128, 128, E4M3FN, 1e-8, None) == -1
    assert qnt(p + 2, p, 4, 128, 128, 128, E4M3FN, 1e-8, None) == -1
    assert qnth(p + 1, p, F16, F16, 4, 128, 128, 128, E4M3FN, 1e-8, None) == -1
    assert qnth(p, p + 2, F16, F32, 4, 128, 128, 128, E4M3FN, 1e-8, None) == -1
    # types: a half entry takes half types, quantize's y_type is float32 or x_type
    assert ench(p, p, p, F32, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert ench(p, p, p, 3, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert dech(p, p, p, F32, 4, 128, 1, 128, E4M3FN, None) == -1
    assert dech(p, p, p, 3, 4, 128, 1, 128, E4M3FN, None) == -1
    assert qnth(p, p, F32, F32, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert qnth(p, p, F16, BF16, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    assert qnth(p, p, BF16, F16, 4, 128, 1, 128, E4M3FN, 1e-8, None) == -1
    # any other format, any other tile
    for fmt in (2, -1, 7):
        assert enc(p, p, p, 4, 128, 1, 128, fmt, 1e-8, None) == -2
        assert dech(p, p, p, F16, 4, 128, 128, 1, fmt, None) == -2
        assert qnth(p, p, BF16, BF16, 4, 128, 128, 128, fmt, 1e-8, None) == -2
    for tr, tk in ((1, 1), (1, 64), (64, 64), (128, 64), (1, 256), (0, 128), (128, 0), (-1, 128), (32, 1), (128, 2)):
        assert enc(p, p, p, 4, 128, tr, tk, E4M3FN, 1e-8, None) == -2, (tr, tk)
        assert ench(p, p, p, BF16, 4, 128, tr, tk, E5M2, 1e-8, None) == -2, (tr, tk)
        assert dec(p, p, p, 4, 128, tr, tk, E4M3FN, None) == -2, (tr, tk)
        assert qnt(p, p, 4, 128, tr, tk, E4M3FN, 1e-8, None) == -2, (tr, tk)
        assert L.fp8q_ocpb_route(4, 128, tr, tk, F32, 1) == -2, (tr, tk)


def test_route_answers_without_a_gpu():
    import fp8q
    from fp8q import ops
    route = fp8q.lib().fp8q_ocpb_route
    for xt in (F32, F16, BF16):
        assert route(7, 384, 1, 128, xt, 1) == ROWS
        assert route(7, 385, 1, 128, xt, 1) == PLAIN and route(7, 127, 1, 128, xt, 1) == PLAIN
        assert route(7, 384, 1, 128, xt, 0) == PLAIN
        for tr, tk in ((128, 1), (128, 128)):
            assert route(256, 384, tr, tk, xt, 1) == PANEL and route(130, 260, tr, tk, xt, 1) == PANEL
            assert route(1, 4, tr, tk, xt, 1) == PANEL
            assert route(256, 383, tr, tk, xt, 1) == PLAIN and route(130, 257, tr, tk, xt, 1) == PLAIN
            assert route(256, 384, tr, tk, xt, 0) == PLAIN
    assert route(0, 128, 1, 128, F32, 1) == -1 and route(4, 0, 1, 128, F32, 1) == -1 and route(4, 128, 1, 128, 3, 1) == -1
    assert route(1 << 62, 4, 1, 128, F32, 1) == -1
    assert ops.OCP_BLOCK_KERNELS == ("rows", "panel", "plain") and ops.OCP_BLOCK_TILES == ob.TILES
    assert ops.ocp_block_route(7, 384, (1, 128), torch.float32) == "rows"
    assert ops.ocp_block_route(7, 384, [128, 128], torch.bfloat16) == "panel"
    assert ops.ocp_block_route(7, 384, (128, 1), torch.float16, aligned16=False) == "plain"
    with pytest.raises(ops.Fp8qError, match="tile must be"):
        ops.ocp_block_route(7, 384, (64, 64), torch.float32)
    with pytest.raises(ops.Fp8qError, match="dtype must be"):
        ops.ocp_block_route(7, 384, (1, 128), torch.float64)
    with pytest.raises(ops.Fp8qError):
        ops.ocp_block_route(0, 384, (1, 128), torch.float32)


@pytest.mark.parametrize("tile", ob.TILES)
@pytest.mark.parametrize("fmt", FMTS)
def test_ops_raise_on_cpu_tensors(fmt, tile):
    from fp8q import ops
    x = torch.randn(4, 256)
    with pytest.raises(ops.Fp8qError, match="no CPU path"):
        ops.ocp_block_encode(x, fmt, tile)
    with pytest.raises(ops.Fp8qError, match="no CPU path"):
        ops.ocp_block_quantize(x.bfloat16(), fmt, tile)
    codes = torch.zeros(4, 256, dtype=torch.uint8)
    scales = torch.ones(ob.oracle(x, fmt, tile)[1].shape)
    with pytest.raises(ops.Fp8qError, match="no CPU path"):
        ops.ocp_block_decode(codes.view(fmt), scales, tile)
    with pytest.raises(ops.Fp8qError, match="no CPU path"):
        ops.ocp_block_decode(codes, scales, tile, fmt=fmt)


def test_ops_refuse_bad_tiles_formats_shapes_and_scales():
    from fp8q import ops
    x = torch.randn(4, 256)
    fmt = torch.float8_e4m3fn
    for tile in ((64, 64), (1, 32), (128,), None, 128, (128, 128, 1), (True, 128)):
        with pytest.raises(ops.Fp8qError, match="tile must be"):
            ops.ocp_block_encode(x, fmt, tile)
        with pytest.raises(ops.Fp8qError, match="tile must be"):
            ops.ocp_block_quantize(x, fmt, tile)
        with pytest.raises(ops.Fp8qError, match="tile must be"):
            ops.ocp_block_decode(torch.zeros(4, 256, dtype=fmt), torch.ones(4, 2), tile)
    for bad in (torch.float16, torch.uint8, torch.float4_e2m1fn_x2, getattr(torch, "float8_e4m3fnuz", torch.int8), "e2m3"):
        with pytest.raises(ops.Fp8qError, match="fmt must be"):
            ops.ocp_block_encode(x, bad)
        with pytest.raises(ops.Fp8qError, match="fmt must be"):
            ops.ocp_block_quantize(x, bad, (128, 128))
    # the tiles that span rows are those of a matrix; (1, 128) takes any rank but not a scalar
    for tile in ((128, 1), (128, 128)):
        with pytest.raises(ops.Fp8qError, match="2-D"):
            ops.ocp_block_encode(torch.randn(2, 3, 128), fmt, tile)
        with pytest.raises(ops.Fp8qError, match="2-D"):
            ops.ocp_block_quantize(torch.randn(128), fmt, tile)
    with pytest.raises(ops.Fp8qError, match="at least one"):
        ops.ocp_block_encode(torch.tensor(1.0), fmt)
    # wrong scale shapes are told from the shapes alone
    c = torch.zeros(130, 260, dtype=fmt)
    for tile, good in (((1, 128), (130, 3)), ((128, 1), (2, 260)), ((128, 128), (2, 3))):
        assert ob.oracle(torch.zeros(130, 260), fmt, tile)[1].shape == good
        for shape in ((good[0] + 1, good[1]), (good[0], good[1] + 1), (good[0] * good[1],), good[::-1]):
            with pytest.raises(ops.Fp8qError, match="scales are"):
                ops.ocp_block_decode(c, torch.ones(shape), tile)
    assert ops._ocpb_geometry((2, 3, 260), (1, 128)) == (6, 260, (2, 3, 3))
    with pytest.raises(ops.Fp8qError):                      # a half decode target exists, an integer one does not
        ops.ocp_block_decode(c, torch.ones(130, 3), out_dtype=torch.int32)
    with pytest.raises(ops.Fp8qError):                      # uint8 codes without fmt=, and on the CPU at that
        ops.ocp_block_decode(torch.zeros(130, 260, dtype=torch.uint8), torch.ones(130, 3))


def test_quantizer_protocol_registry_and_constructor():
    from quantization.fp8 import QuantizerBase
    from quantization.manager import QMethods
    from quantization.ocp import OCPBlockFP8Quantizer as Q
    assert issubclass(Q, QuantizerBase) and Q.range_free is True
    assert QMethods.list_names() == ["symmetric_uniform", "asymmetric_uniform", "fp_quantizer"]
    assert all(m.cls is not Q for m in QMethods)
    q = Q()
    assert q.n_bits == 8 and q.fmt == torch.float8_e4m3fn and q.tile == (1, 128) and q.eps == 1e-8
    assert not q.keep_dtype and not q.flatten_rows and q.fmax == 448.0
    assert q.is_initialized is True and q.symmetric is True
    q.set_quant_range(torch.tensor(-1.0), torch.tensor(1.0))          # no-ops: there is no range
    q.reset()
    q.fix_ranges()
    assert q.is_initialized is True
    q2 = Q(fmt=torch.float8_e5m2, tile=[128, 128], eps=1e-4, flatten_rows=True, per_channel=True, scale_domain="linear")
    assert q2.tile == (128, 128) and q2.fmax == 57344.0
    assert "E5M2" in q2.extra_repr() and "128x128" in q2.extra_repr() and "0.0001" in q2.extra_repr()
    for kw in (dict(n_bits=4), dict(fmt=torch.float16), dict(fmt=torch.float4_e2m1fn_x2), dict(tile=(64, 64)),
               dict(tile=(1, 32)), dict(tile=128), dict(eps=-1.0), dict(eps="tiny")):
        with pytest.raises(ValueError):
            Q(**kw)
    # flatten_rows: [shape[0], -1] for more than two dimensions, the tensor itself otherwise
    w = torch.zeros(8, 3, 3, 3)
    assert tuple(q2._rows(w).shape) == (8, 27) and q2._rows(w[0, 0]).shape == (3, 3) and q._rows(w).shape == w.shape


def test_quantizer_is_forward_only():
    from quantization.ocp import OCPBlockFP8Quantizer
    q = OCPBlockFP8Quantizer()
    with pytest.raises(NotImplementedError):
        q(torch.randn(4, 128, requires_grad=True))
    with pytest.raises(NotImplementedError):
        q.make_range_trainable()


def test_manager_never_gives_the_estimator_work():
    """in every state a range_free quantizer is called directly: the estimator object the manager builds is never called (a
    CPU tensor gets as far as the op's refusal, which is behind the point where an estimator would have run)"""
    from fp8q import ops
    from quantization.estimators import RangeEstimators
    from quantization.manager import QuantizationManager
    from quantization.ocp import OCPBlockFP8Quantizer
    mgr = QuantizationManager(qmethod=OCPBlockFP8Quantizer, init=RangeEstimators.current_minmax.cls, per_channel=True,
                              qparams=dict(n_bits=8, scale_domain="linear", fmt=torch.float8_e5m2, tile=(128, 128)))
    assert isinstance(mgr.quantizer, OCPBlockFP8Quantizer) and mgr.quantizer.tile == (128, 128)
    calls = []
    mgr.range_estimator.register_forward_pre_hook(lambda m, a: calls.append(a))
    seen = []
    mgr.quantizer.register_forward_pre_hook(lambda m, a: seen.append(a[0].dtype))
    for enter in (mgr.estimate_ranges, mgr.estimate_ranges_train, mgr.fix_ranges):      # fix_ranges: always initialized
        enter()
        for x in (torch.randn(4, 128), torch.randn(4, 128).bfloat16()):
            with pytest.raises(ops.Fp8qError):
                mgr(x)
    assert calls == []
    assert seen == [torch.float32, torch.bfloat16] * 3           # half tensors reach the quantizer as they are
    mgr.reset_ranges()
    assert mgr.quantizer.is_initialized


def test_the_oracle_has_the_contracts_properties():
    """[130, 257] with a planted infinity, a NaN and a zero tile: the shapes of the three scale tables, what inf / NaN / zero
    tiles give, and 128x1 of x == the transpose of 1x128 of x.t()"""
    fmt = torch.float8_e4m3fn
    g = torch.Generator().manual_seed(0)
    x = torch.randn(130, 257, generator=g)
    x[0, 0] = float("inf")
    x[3, 130] = float("nan")
    x[128:, 128:256] = 0.0
    shapes = {(1, 128): (130, 3), (128, 1): (2, 257), (128, 128): (2, 3)}
    for tile, sshape in shapes.items():
        c, s, v = ob.oracle(x, fmt, tile)
        assert s.shape == sshape and c.shape == x.shape and c.dtype == fmt and v.shape == x.shape
    c, s, v = ob.oracle(x, fmt, (128, 128))
    cb = c.view(torch.uint8)
    assert torch.isinf(s[0, 0]) and cb[0, 0] == 0x7F and (cb[:128, :128].flatten()[1:] & 0x7F == 0).all()
    assert torch.isnan(v[:128, :128]).all()
    assert torch.isnan(s[0, 1]) and (cb[:128, 128:256] == 0x7F).all()
    assert s[1, 1].item() == (torch.tensor(1e-8) / 448.0).item() and (cb[128:, 128:256] == 0).all()
    ccol, scol, _ = ob.oracle(x, fmt, (128, 1))
    crow, srow, _ = ob.oracle(x.t().contiguous(), fmt, (1, 128))
    assert torch.equal(ccol.view(torch.uint8), crow.view(torch.uint8).t())
    ob.same(scol, srow.t().contiguous(), "scales")
    # the planted case of the GPU tests: a zero tile, a NaN tile and an infinite one where there are tiles enough
    x = ob.case((130, 260), fmt, (128, 128))
    s = ob.oracle(x, fmt, (128, 128))[1].flatten()
    assert s[1].item() == (torch.tensor(1e-8) / 448.0).item() and torch.isnan(s[2]) and torch.isinf(s[3])
