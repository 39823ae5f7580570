"""CPU-only checks of the tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block.hip): the library exports its seven entry points
and reports every argument error before any launch, fp8q_ocpb_route answers without a GPU, the Python wrappers refuse CPU
tensors, bad tiles, bad formats and wrong scale shapes (there is no fallback), OCPBlockFP8Quantizer follows the quantizer
protocol without being one of the CLI's methods or ever giving its manager's estimator work, and the oracle the GPU tests use
has the properties the contract states; and (the last section) the inputs of tests/test_ocpb_ties_gpu.py do take the redo of
csrc/fp8q_ocpq.h, counted tile by tile."""
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


# ---- the inputs of tests/test_ocpb_ties_gpu.py ---------------------------------------------------------------------------
# Conditions on the inputs of tests/test_ocpb_ties_gpu.py, checked on the CPU so that those tests cannot pass vacuously: the
# tiles of ocpb_oracle.tie_case do take the redo of csrc/fp8q_ocpq.h (code4 / code1: the two ends of the error interval around
# x * fl(1/s) disagree, or the product is NaN), and a kernel without the redo would get some of them wrong.  Nothing here needs
# a GPU or calls the library: ocpb_oracle.redo_counts restates the decision in torch's CPU arithmetic.
#
# For every (tile, shape, format, dtype) of the GPU tests, and for every range kind (ocpb_oracle.TIE_KINDS) that has a tile of
# more than two elements there (a tile of one or two holds +m and -m alone, the rule that makes its amax exact):
#   * float32: some tile of the kind has an element that takes the redo, and some tile of an inexact scale (3.0, 0.7) has an
#     element whose code is wrong without it;
#   * every tile of the 1e-37 kind has a subnormal scale whose reciprocal is infinite, and ALL its elements take the redo;
#   * float16 / bfloat16: the 65536 patterns of the dtype were searched under the kind's scale (ocpb_oracle.half_search; SEARCH
#     below holds how many patterns take the redo and how many are wrong without it).  Where no pattern of the dtype takes the
#     redo, no tensor of that dtype can, and the test asserts exactly that (counts of 0): float16 under 0.7 and under its
#     smallest subnormal (which stands where 1e-37 cannot: nothing overflows in float16), and under 3.0 with E5M2.  Where
#     patterns take it but none is wrong without it -- every other range of both half dtypes but one -- "takes the redo" is
#     the condition; where some are wrong without it (bfloat16's 1e-37), "wrong without" is asserted too.
# COUNTS holds, for every case, (elements that take the redo, elements wrong without it, tiles of more than two elements) summed
# over the tiles of each kind, in the order of TIE_KINDS; the test asserts these very numbers, so a change of tie_case, of the
# ranges or of the shapes is noticed here.  The sums in float32 at (128, 128) agree with the per-tensor midpoint set: 66 of its
# 1009 (E4M3FN) / 985 (E5M2) elements are wrong without the redo under 3.0, none under fmax * 2^-5, all under 1e-37.
from ocpb_oracle import COL, FMAX, FULL, ROW, TIE_EPS, TIE_KINDS       # noqa: E402

_id = {torch.float8_e4m3fn: "e4m3fn", torch.float8_e5m2: "e5m2", torch.float32: "f32", torch.float16: "f16",
       torch.bfloat16: "bf16", ROW: "row", COL: "col", FULL: "full"}
INEXACT, OVERFLOW = (0, 3), 2
# the inputs of the nontemporal tests that tie_case makes: (format, tile, dtype), whole panels from two points of the rotation
NT_PANELS = [(torch.float8_e4m3fn, ROW, torch.float32), (torch.float8_e5m2, COL, torch.float32),
             (torch.float8_e4m3fn, FULL, torch.float32), (torch.float8_e5m2, FULL, torch.bfloat16)]
EPS0 = [(ROW, (3, 256)), (COL, (130, 260)), (FULL, (130, 260)), (FULL, (130, 257))]


def cases():
    """(name, x, format, tile, dtype, seed) of every tie_case tensor the GPU tests make"""
    def name(family, tile, shape, fmt, dtype):
        return f"{family} {_id[tile]} {shape[0]}x{shape[1]} {_id[fmt]} {_id[dtype]}"

    for fmt in FMTS:
        for dtype in ob.TIE_DTYPES:
            for tile, shape, _ in ob.TIE_LANE_CASES:
                yield name("lane", tile, shape, fmt, dtype), ob.tie_case(shape, fmt, tile, dtype), fmt, tile, dtype, 0
            for (R, K) in ob.TIE_T_SHAPES:              # planted row-wise, and on the transpose: tie_case of [K, R]
                for tile in (ROW, FULL):
                    for shape in ((R, K), (K, R)):
                        yield name("t", tile, shape, fmt, dtype), ob.tie_case(shape, fmt, tile, dtype), fmt, tile, dtype, 0
        for dtype in (torch.float32, torch.bfloat16):
            for tile, shape in EPS0:
                yield name("eps0", tile, shape, fmt, dtype), ob.tie_case(shape, fmt, tile, dtype), fmt, tile, dtype, 0
    for fmt, tile, dtype in NT_PANELS:
        for seed in (0, 1):
            yield (name(f"nt{seed}", tile, (128, 128), fmt, dtype), ob.tie_case((128, 128), fmt, tile, dtype, seed), fmt, tile,
                   dtype, seed)


def counts_by_kind(x, fmt, tile, seed=0):
    """((taken, wrong_without, tiles of more than two elements) summed over the tiles of each kind, in TIE_KINDS' order)"""
    tr, tk = tile
    R, K = x.shape
    kinds = ob.tie_kind_of_tiles(x.shape, tile, seed)
    taken, wrong = ob.redo_counts(x, fmt, tile, TIE_EPS)
    h = torch.clamp(R - tr * torch.arange(kinds.shape[0]), max=tr).view(-1, 1)
    w = torch.clamp(K - tk * torch.arange(kinds.shape[1]), max=tk).view(1, -1)
    big = h * w > 2
    return tuple((int(taken[(kinds == k) & big].sum()), int(wrong[(kinds == k) & big].sum()), int(((kinds == k) & big).sum()))
                 for k in range(len(TIE_KINDS)))


# patterns of a half dtype (of 65536) that (take the redo, are wrong without it), per kind in TIE_KINDS' order
SEARCH = {
    "e4m3fn f16": ((32, 0), (252, 0), (0, 0), (0, 0), (32, 0)),
    "e4m3fn bf16": ((32, 0), (252, 0), (1042, 1042), (2, 0), (2, 0)),
    "e5m2 f16": ((0, 0), (246, 0), (0, 0), (0, 0), (2, 0)),
    "e5m2 bf16": ((2, 0), (246, 0), (1042, 1042), (2, 0), (2, 0)),
}

COUNTS = {
    "lane row 9x1024 e4m3fn f32": ((1414, 122, 15), (1414, 0, 15), (1792, 1792, 14), (1319, 48, 14), (1319, 114, 14)),
    "lane row 40x256 e4m3fn f32": ((1510, 132, 16), (1510, 0, 16), (2048, 2048, 16), (1510, 57, 16), (1510, 128, 16)),
    "lane row 3x130 e4m3fn f32": ((95, 8, 1), (0, 0, 0), (128, 128, 1), (0, 0, 0), (95, 11, 1)),
    "lane col 136x264 e4m3fn f32": ((5239, 451, 106), (5239, 0, 106), (7208, 7208, 106), (5234, 198, 105), (5144, 439, 105)),
    "lane col 256x384 e4m3fn f32": ((14537, 1262, 154), (14537, 0, 154), (19712, 19712, 154), (14442, 537, 153), (14442, 1225, 153)),
    "lane col 130x257 e4m3fn f32": ((4907, 428, 52), (4907, 0, 52), (6528, 6528, 51), (4814, 179, 51), (4814, 412, 51)),
    "lane full 136x264 e4m3fn f32": ((12321, 1070, 2), (12275, 0, 1), (1024, 1024, 1), (766, 28, 1), (766, 65, 1)),
    "lane full 256x384 e4m3fn f32": ((24549, 2137, 2), (12275, 0, 1), (16384, 16384, 1), (12275, 455, 1), (12275, 1045, 1)),
    "lane full 130x257 e4m3fn f32": ((12275, 1068, 1), (12275, 0, 1), (128, 128, 1), (190, 7, 1), (190, 21, 1)),
    "t row 144x260 e4m3fn f32": ((5515, 480, 87), (5519, 0, 87), (7412, 7412, 86), (5419, 202, 86), (5518, 467, 86)),
    "t row 260x144 e4m3fn f32": ((5457, 464, 104), (5447, 0, 104), (7488, 7488, 104), (5447, 199, 104), (5457, 453, 104)),
    "t full 144x260 e4m3fn f32": ((12321, 1070, 2), (12275, 0, 1), (512, 512, 1), (1534, 57, 1), (1534, 129, 1)),
    "t full 260x144 e4m3fn f32": ((12321, 1070, 2), (1534, 0, 1), (16384, 16384, 1), (1534, 57, 1), (381, 36, 1)),
    "t row 132x132 e4m3fn f32": ((2591, 223, 53), (2494, 0, 53), (3560, 3560, 53), (2494, 95, 53), (2496, 221, 52)),
    "t row 132x132 e4m3fn f32": ((2591, 223, 53), (2494, 0, 53), (3560, 3560, 53), (2494, 95, 53), (2496, 221, 52)),
    "t full 132x132 e4m3fn f32": ((12275, 1068, 1), (381, 0, 1), (512, 512, 1), (11, 0, 1), (0, 0, 0)),
    "t full 132x132 e4m3fn f32": ((12275, 1068, 1), (381, 0, 1), (512, 512, 1), (11, 0, 1), (0, 0, 0)),
    "t row 130x260 e4m3fn f32": ((4944, 429, 78), (4948, 0, 78), (6760, 6760, 78), (4944, 185, 78), (4948, 418, 78)),
    "t row 260x130 e4m3fn f32": ((4914, 415, 52), (4901, 0, 52), (6656, 6656, 52), (4901, 178, 52), (4914, 409, 52)),
    "t full 130x260 e4m3fn f32": ((12280, 1068, 2), (12275, 0, 1), (512, 512, 1), (190, 7, 1), (190, 21, 1)),
    "t full 260x130 e4m3fn f32": ((12280, 1068, 2), (190, 0, 1), (16384, 16384, 1), (190, 7, 1), (381, 36, 1)),
    "t row 129x131 e4m3fn f32": ((2476, 215, 52), (2473, 0, 52), (3406, 3406, 52), (2380, 88, 51), (2475, 221, 51)),
    "t row 131x129 e4m3fn f32": ((2550, 220, 27), (2452, 0, 26), (3328, 3328, 26), (2452, 91, 26), (2455, 218, 26)),
    "t full 129x131 e4m3fn f32": ((12275, 1068, 1), (286, 0, 1), (128, 128, 1), (1, 0, 1), (0, 0, 0)),
    "t full 131x129 e4m3fn f32": ((12275, 1068, 1), (95, 0, 1), (384, 384, 1), (1, 0, 1), (0, 0, 0)),
    "lane row 9x1024 e4m3fn f16": ((378, 0, 15), (1414, 0, 15), (0, 0, 14), (0, 0, 14), (378, 0, 14)),
    "lane row 40x256 e4m3fn f16": ((410, 0, 16), (1510, 0, 16), (0, 0, 16), (0, 0, 16), (410, 0, 16)),
    "lane row 3x130 e4m3fn f16": ((32, 0, 1), (0, 0, 0), (0, 0, 1), (0, 0, 0), (32, 0, 1)),
    "lane col 136x264 e4m3fn f16": ((1422, 0, 106), (5239, 0, 106), (0, 0, 106), (0, 0, 105), (1384, 0, 105)),
    "lane col 256x384 e4m3fn f16": ((3906, 0, 154), (14537, 0, 154), (0, 0, 154), (0, 0, 153), (3876, 0, 153)),
    "lane col 130x257 e4m3fn f16": ((1324, 0, 52), (4907, 0, 52), (0, 0, 51), (0, 0, 51), (1292, 0, 51)),
    "lane full 136x264 e4m3fn f16": ((3326, 0, 2), (12275, 0, 1), (0, 0, 1), (0, 0, 1), (224, 0, 1)),
    "lane full 256x384 e4m3fn f16": ((6590, 0, 2), (12275, 0, 1), (0, 0, 1), (0, 0, 1), (3296, 0, 1)),
    "lane full 130x257 e4m3fn f16": ((3296, 0, 1), (12275, 0, 1), (0, 0, 1), (0, 0, 1), (64, 0, 1)),
    "t row 144x260 e4m3fn f16": ((1492, 0, 87), (5519, 0, 87), (0, 0, 86), (0, 0, 86), (1462, 0, 86)),
    "t row 260x144 e4m3fn f16": ((1464, 0, 104), (5447, 0, 104), (0, 0, 104), (0, 0, 104), (1464, 0, 104)),
    "t full 144x260 e4m3fn f16": ((3326, 0, 2), (12275, 0, 1), (0, 0, 1), (0, 0, 1), (416, 0, 1)),
    "t full 260x144 e4m3fn f16": ((3326, 0, 2), (1534, 0, 1), (0, 0, 1), (0, 0, 1), (126, 0, 1)),
    "t row 132x132 e4m3fn f16": ((704, 0, 53), (2494, 0, 53), (0, 0, 53), (0, 0, 53), (672, 0, 52)),
    "t row 132x132 e4m3fn f16": ((704, 0, 53), (2494, 0, 53), (0, 0, 53), (0, 0, 53), (672, 0, 52)),
    "t full 132x132 e4m3fn f16": ((3296, 0, 1), (381, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 0)),
    "t full 132x132 e4m3fn f16": ((3296, 0, 1), (381, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 0)),
    "t row 130x260 e4m3fn f16": ((1334, 0, 78), (4948, 0, 78), (0, 0, 78), (0, 0, 78), (1334, 0, 78)),
    "t row 260x130 e4m3fn f16": ((1324, 0, 52), (4901, 0, 52), (0, 0, 52), (0, 0, 52), (1324, 0, 52)),
    "t full 130x260 e4m3fn f16": ((3296, 0, 2), (12275, 0, 1), (0, 0, 1), (0, 0, 1), (64, 0, 1)),
    "t full 260x130 e4m3fn f16": ((3296, 0, 2), (190, 0, 1), (0, 0, 1), (0, 0, 1), (126, 0, 1)),
    "t row 129x131 e4m3fn f16": ((667, 0, 52), (2473, 0, 52), (0, 0, 52), (0, 0, 51), (667, 0, 51)),
    "t row 131x129 e4m3fn f16": ((694, 0, 27), (2452, 0, 26), (0, 0, 26), (0, 0, 26), (662, 0, 26)),
    "t full 129x131 e4m3fn f16": ((3296, 0, 1), (286, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 0)),
    "t full 131x129 e4m3fn f16": ((3296, 0, 1), (95, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 0)),
    "lane row 9x1024 e4m3fn bf16": ((378, 0, 15), (1414, 0, 15), (1792, 1792, 14), (28, 0, 14), (28, 0, 14)),
    "lane row 40x256 e4m3fn bf16": ((410, 0, 16), (1510, 0, 16), (2048, 2048, 16), (32, 0, 16), (32, 0, 16)),
    "lane row 3x130 e4m3fn bf16": ((32, 0, 1), (0, 0, 0), (128, 128, 1), (0, 0, 0), (2, 0, 1)),
    "lane col 136x264 e4m3fn bf16": ((1422, 0, 106), (5239, 0, 106), (7208, 7208, 106), (112, 0, 105), (110, 0, 105)),
    "lane col 256x384 e4m3fn bf16": ((3906, 0, 154), (14537, 0, 154), (19712, 19712, 154), (298, 0, 153), (298, 0, 153)),
    "lane col 130x257 e4m3fn bf16": ((1324, 0, 52), (4907, 0, 52), (6528, 6528, 51), (102, 0, 51), (102, 0, 51)),
    "lane full 136x264 e4m3fn bf16": ((3326, 0, 2), (12275, 0, 1), (1024, 1024, 1), (16, 0, 1), (16, 0, 1)),
    "lane full 256x384 e4m3fn bf16": ((6590, 0, 2), (12275, 0, 1), (16384, 16384, 1), (254, 0, 1), (254, 0, 1)),
    "lane full 130x257 e4m3fn bf16": ((3296, 0, 1), (12275, 0, 1), (128, 128, 1), (4, 0, 1), (4, 0, 1)),
    "t row 144x260 e4m3fn bf16": ((1492, 0, 87), (5519, 0, 87), (7412, 7412, 86), (112, 0, 86), (114, 0, 86)),
    "t row 260x144 e4m3fn bf16": ((1464, 0, 104), (5447, 0, 104), (7488, 7488, 104), (116, 0, 104), (116, 0, 104)),
    "t full 144x260 e4m3fn bf16": ((3326, 0, 2), (12275, 0, 1), (512, 512, 1), (32, 0, 1), (32, 0, 1)),
    "t full 260x144 e4m3fn bf16": ((3326, 0, 2), (1534, 0, 1), (16384, 16384, 1), (32, 0, 1), (8, 0, 1)),
    "t row 132x132 e4m3fn bf16": ((704, 0, 53), (2494, 0, 53), (3560, 3560, 53), (54, 0, 53), (52, 0, 52)),
    "t row 132x132 e4m3fn bf16": ((704, 0, 53), (2494, 0, 53), (3560, 3560, 53), (54, 0, 53), (52, 0, 52)),
    "t full 132x132 e4m3fn bf16": ((3296, 0, 1), (381, 0, 1), (512, 512, 1), (2, 0, 1), (0, 0, 0)),
    "t full 132x132 e4m3fn bf16": ((3296, 0, 1), (381, 0, 1), (512, 512, 1), (2, 0, 1), (0, 0, 0)),
    "t row 130x260 e4m3fn bf16": ((1334, 0, 78), (4948, 0, 78), (6760, 6760, 78), (102, 0, 78), (102, 0, 78)),
    "t row 260x130 e4m3fn bf16": ((1324, 0, 52), (4901, 0, 52), (6656, 6656, 52), (102, 0, 52), (102, 0, 52)),
    "t full 130x260 e4m3fn bf16": ((3296, 0, 2), (12275, 0, 1), (512, 512, 1), (4, 0, 1), (4, 0, 1)),
    "t full 260x130 e4m3fn bf16": ((3296, 0, 2), (190, 0, 1), (16384, 16384, 1), (4, 0, 1), (8, 0, 1)),
    "t row 129x131 e4m3fn bf16": ((667, 0, 52), (2473, 0, 52), (3406, 3406, 52), (51, 0, 51), (52, 0, 51)),
    "t row 131x129 e4m3fn bf16": ((694, 0, 27), (2452, 0, 26), (3328, 3328, 26), (52, 0, 26), (52, 0, 26)),
    "t full 129x131 e4m3fn bf16": ((3296, 0, 1), (286, 0, 1), (128, 128, 1), (1, 0, 1), (0, 0, 0)),
    "t full 131x129 e4m3fn bf16": ((3296, 0, 1), (95, 0, 1), (384, 384, 1), (1, 0, 1), (0, 0, 0)),
    "eps0 row 3x256 e4m3fn f32": ((189, 14, 2), (95, 0, 1), (128, 128, 1), (95, 3, 1), (95, 11, 1)),
    "eps0 col 130x260 e4m3fn f32": ((4907, 428, 52), (4907, 0, 52), (6656, 6656, 52), (4907, 182, 52), (4907, 420, 52)),
    "eps0 full 130x260 e4m3fn f32": ((12280, 1068, 2), (12275, 0, 1), (512, 512, 1), (190, 7, 1), (190, 21, 1)),
    "eps0 full 130x257 e4m3fn f32": ((12275, 1068, 1), (12275, 0, 1), (128, 128, 1), (190, 7, 1), (190, 21, 1)),
    "eps0 row 3x256 e4m3fn bf16": ((64, 0, 2), (95, 0, 1), (128, 128, 1), (2, 0, 1), (2, 0, 1)),
    "eps0 col 130x260 e4m3fn bf16": ((1324, 0, 52), (4907, 0, 52), (6656, 6656, 52), (104, 0, 52), (104, 0, 52)),
    "eps0 full 130x260 e4m3fn bf16": ((3296, 0, 2), (12275, 0, 1), (512, 512, 1), (4, 0, 1), (4, 0, 1)),
    "eps0 full 130x257 e4m3fn bf16": ((3296, 0, 1), (12275, 0, 1), (128, 128, 1), (4, 0, 1), (4, 0, 1)),
    "lane row 9x1024 e5m2 f32": ((1417, 127, 15), (1417, 0, 15), (1792, 1792, 14), (1322, 0, 14), (1322, 111, 14)),
    "lane row 40x256 e5m2 f32": ((1513, 137, 16), (1513, 0, 16), (2048, 2048, 16), (1513, 0, 16), (1513, 126, 16)),
    "lane row 3x130 e5m2 f32": ((94, 11, 1), (0, 0, 0), (128, 128, 1), (0, 0, 0), (94, 7, 1)),
    "lane col 136x264 e5m2 f32": ((5241, 472, 106), (5241, 0, 106), (7208, 7208, 106), (5238, 0, 105), (5149, 434, 105)),
    "lane col 256x384 e5m2 f32": ((14538, 1300, 154), (14538, 0, 154), (19712, 19712, 154), (14444, 0, 153), (14444, 1214, 153)),
    "lane col 130x257 e5m2 f32": ((4909, 442, 52), (4909, 0, 52), (6528, 6528, 51), (4814, 0, 51), (4814, 405, 51)),
    "lane full 136x264 e5m2 f32": ((12322, 1106, 2), (12274, 0, 1), (1024, 1024, 1), (766, 0, 1), (766, 64, 1)),
    "lane full 256x384 e5m2 f32": ((24549, 2200, 2), (12274, 0, 1), (16384, 16384, 1), (12274, 0, 1), (12274, 1031, 1)),
    "lane full 130x257 e5m2 f32": ((12274, 1102, 1), (12274, 0, 1), (128, 128, 1), (189, 0, 1), (189, 16, 1)),
    "t row 144x260 e5m2 f32": ((5518, 493, 87), (5518, 0, 87), (7412, 7412, 86), (5424, 0, 86), (5516, 464, 86)),
    "t row 260x144 e5m2 f32": ((5465, 491, 104), (5445, 0, 104), (7488, 7488, 104), (5445, 0, 104), (5465, 462, 104)),
    "t full 144x260 e5m2 f32": ((12322, 1106, 2), (12274, 0, 1), (512, 512, 1), (1534, 0, 1), (1534, 128, 1)),
    "t full 260x144 e5m2 f32": ((12322, 1106, 2), (1534, 0, 1), (16384, 16384, 1), (1534, 0, 1), (383, 32, 1)),
    "t row 132x132 e5m2 f32": ((2580, 234, 53), (2502, 0, 53), (3560, 3560, 53), (2502, 0, 53), (2486, 211, 52)),
    "t row 132x132 e5m2 f32": ((2580, 234, 53), (2502, 0, 53), (3560, 3560, 53), (2502, 0, 53), (2486, 211, 52)),
    "t full 132x132 e5m2 f32": ((12274, 1102, 1), (383, 0, 1), (512, 512, 1), (10, 0, 1), (0, 0, 0)),
    "t full 132x132 e5m2 f32": ((12274, 1102, 1), (383, 0, 1), (512, 512, 1), (10, 0, 1), (0, 0, 0)),
    "t row 130x260 e5m2 f32": ((4948, 441, 78), (4946, 0, 78), (6760, 6760, 78), (4948, 0, 78), (4946, 414, 78)),
    "t row 260x130 e5m2 f32": ((4906, 444, 52), (4913, 0, 52), (6656, 6656, 52), (4913, 0, 52), (4906, 412, 52)),
    "t full 130x260 e5m2 f32": ((12279, 1103, 2), (12274, 0, 1), (512, 512, 1), (189, 0, 1), (189, 16, 1)),
    "t full 260x130 e5m2 f32": ((12279, 1103, 2), (189, 0, 1), (16384, 16384, 1), (189, 0, 1), (383, 32, 1)),
    "t row 129x131 e5m2 f32": ((2467, 226, 52), (2481, 0, 52), (3406, 3406, 52), (2386, 0, 51), (2466, 209, 51)),
    "t row 131x129 e5m2 f32": ((2544, 231, 27), (2459, 0, 26), (3328, 3328, 26), (2459, 0, 26), (2450, 207, 26)),
    "t full 129x131 e5m2 f32": ((12274, 1102, 1), (286, 0, 1), (128, 128, 1), (1, 0, 1), (0, 0, 0)),
    "t full 131x129 e5m2 f32": ((12274, 1102, 1), (94, 0, 1), (384, 384, 1), (1, 0, 1), (0, 0, 0)),
    "lane row 9x1024 e5m2 f16": ((0, 0, 15), (1417, 0, 15), (0, 0, 14), (0, 0, 14), (28, 0, 14)),
    "lane row 40x256 e5m2 f16": ((0, 0, 16), (1513, 0, 16), (0, 0, 16), (0, 0, 16), (32, 0, 16)),
    "lane row 3x130 e5m2 f16": ((0, 0, 1), (0, 0, 0), (0, 0, 1), (0, 0, 0), (2, 0, 1)),
    "lane col 136x264 e5m2 f16": ((0, 0, 106), (5241, 0, 106), (0, 0, 106), (0, 0, 105), (110, 0, 105)),
    "lane col 256x384 e5m2 f16": ((0, 0, 154), (14538, 0, 154), (0, 0, 154), (0, 0, 153), (298, 0, 153)),
    "lane col 130x257 e5m2 f16": ((0, 0, 52), (4909, 0, 52), (0, 0, 51), (0, 0, 51), (102, 0, 51)),
    "lane full 136x264 e5m2 f16": ((0, 0, 2), (12274, 0, 1), (0, 0, 1), (0, 0, 1), (16, 0, 1)),
    "lane full 256x384 e5m2 f16": ((0, 0, 2), (12274, 0, 1), (0, 0, 1), (0, 0, 1), (254, 0, 1)),
    "lane full 130x257 e5m2 f16": ((0, 0, 1), (12274, 0, 1), (0, 0, 1), (0, 0, 1), (4, 0, 1)),
    "t row 144x260 e5m2 f16": ((0, 0, 87), (5518, 0, 87), (0, 0, 86), (0, 0, 86), (114, 0, 86)),
    "t row 260x144 e5m2 f16": ((0, 0, 104), (5445, 0, 104), (0, 0, 104), (0, 0, 104), (116, 0, 104)),
    "t full 144x260 e5m2 f16": ((0, 0, 2), (12274, 0, 1), (0, 0, 1), (0, 0, 1), (32, 0, 1)),
    "t full 260x144 e5m2 f16": ((0, 0, 2), (1534, 0, 1), (0, 0, 1), (0, 0, 1), (8, 0, 1)),
    "t row 132x132 e5m2 f16": ((0, 0, 53), (2502, 0, 53), (0, 0, 53), (0, 0, 53), (52, 0, 52)),
    "t row 132x132 e5m2 f16": ((0, 0, 53), (2502, 0, 53), (0, 0, 53), (0, 0, 53), (52, 0, 52)),
    "t full 132x132 e5m2 f16": ((0, 0, 1), (383, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 0)),
    "t full 132x132 e5m2 f16": ((0, 0, 1), (383, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 0)),
    "t row 130x260 e5m2 f16": ((0, 0, 78), (4946, 0, 78), (0, 0, 78), (0, 0, 78), (102, 0, 78)),
    "t row 260x130 e5m2 f16": ((0, 0, 52), (4913, 0, 52), (0, 0, 52), (0, 0, 52), (102, 0, 52)),
    "t full 130x260 e5m2 f16": ((0, 0, 2), (12274, 0, 1), (0, 0, 1), (0, 0, 1), (4, 0, 1)),
    "t full 260x130 e5m2 f16": ((0, 0, 2), (189, 0, 1), (0, 0, 1), (0, 0, 1), (8, 0, 1)),
    "t row 129x131 e5m2 f16": ((0, 0, 52), (2481, 0, 52), (0, 0, 52), (0, 0, 51), (52, 0, 51)),
    "t row 131x129 e5m2 f16": ((0, 0, 27), (2459, 0, 26), (0, 0, 26), (0, 0, 26), (52, 0, 26)),
    "t full 129x131 e5m2 f16": ((0, 0, 1), (286, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 0)),
    "t full 131x129 e5m2 f16": ((0, 0, 1), (94, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 0)),
    "lane row 9x1024 e5m2 bf16": ((30, 0, 15), (1417, 0, 15), (1792, 1792, 14), (28, 0, 14), (28, 0, 14)),
    "lane row 40x256 e5m2 bf16": ((32, 0, 16), (1513, 0, 16), (2048, 2048, 16), (32, 0, 16), (32, 0, 16)),
    "lane row 3x130 e5m2 bf16": ((2, 0, 1), (0, 0, 0), (128, 128, 1), (0, 0, 0), (2, 0, 1)),
    "lane col 136x264 e5m2 bf16": ((112, 0, 106), (5241, 0, 106), (7208, 7208, 106), (112, 0, 105), (110, 0, 105)),
    "lane col 256x384 e5m2 bf16": ((300, 0, 154), (14538, 0, 154), (19712, 19712, 154), (298, 0, 153), (298, 0, 153)),
    "lane col 130x257 e5m2 bf16": ((104, 0, 52), (4909, 0, 52), (6528, 6528, 51), (102, 0, 51), (102, 0, 51)),
    "lane full 136x264 e5m2 bf16": ((256, 0, 2), (12274, 0, 1), (1024, 1024, 1), (16, 0, 1), (16, 0, 1)),
    "lane full 256x384 e5m2 bf16": ((506, 0, 2), (12274, 0, 1), (16384, 16384, 1), (254, 0, 1), (254, 0, 1)),
    "lane full 130x257 e5m2 bf16": ((254, 0, 1), (12274, 0, 1), (128, 128, 1), (4, 0, 1), (4, 0, 1)),
    "t row 144x260 e5m2 bf16": ((114, 0, 87), (5518, 0, 87), (7412, 7412, 86), (112, 0, 86), (114, 0, 86)),
    "t row 260x144 e5m2 bf16": ((116, 0, 104), (5445, 0, 104), (7488, 7488, 104), (116, 0, 104), (116, 0, 104)),
    "t full 144x260 e5m2 bf16": ((256, 0, 2), (12274, 0, 1), (512, 512, 1), (32, 0, 1), (32, 0, 1)),
    "t full 260x144 e5m2 bf16": ((256, 0, 2), (1534, 0, 1), (16384, 16384, 1), (32, 0, 1), (8, 0, 1)),
    "t row 132x132 e5m2 bf16": ((54, 0, 53), (2502, 0, 53), (3560, 3560, 53), (54, 0, 53), (52, 0, 52)),
    "t row 132x132 e5m2 bf16": ((54, 0, 53), (2502, 0, 53), (3560, 3560, 53), (54, 0, 53), (52, 0, 52)),
    "t full 132x132 e5m2 bf16": ((254, 0, 1), (383, 0, 1), (512, 512, 1), (2, 0, 1), (0, 0, 0)),
    "t full 132x132 e5m2 bf16": ((254, 0, 1), (383, 0, 1), (512, 512, 1), (2, 0, 1), (0, 0, 0)),
    "t row 130x260 e5m2 bf16": ((102, 0, 78), (4946, 0, 78), (6760, 6760, 78), (102, 0, 78), (102, 0, 78)),
    "t row 260x130 e5m2 bf16": ((102, 0, 52), (4913, 0, 52), (6656, 6656, 52), (102, 0, 52), (102, 0, 52)),
    "t full 130x260 e5m2 bf16": ((256, 0, 2), (12274, 0, 1), (512, 512, 1), (4, 0, 1), (4, 0, 1)),
    "t full 260x130 e5m2 bf16": ((256, 0, 2), (189, 0, 1), (16384, 16384, 1), (4, 0, 1), (8, 0, 1)),
    "t row 129x131 e5m2 bf16": ((52, 0, 52), (2481, 0, 52), (3406, 3406, 52), (51, 0, 51), (52, 0, 51)),
    "t row 131x129 e5m2 bf16": ((54, 0, 27), (2459, 0, 26), (3328, 3328, 26), (52, 0, 26), (52, 0, 26)),
    "t full 129x131 e5m2 bf16": ((254, 0, 1), (286, 0, 1), (128, 128, 1), (1, 0, 1), (0, 0, 0)),
    "t full 131x129 e5m2 bf16": ((254, 0, 1), (94, 0, 1), (384, 384, 1), (1, 0, 1), (0, 0, 0)),
    "eps0 row 3x256 e5m2 f32": ((188, 21, 2), (94, 0, 1), (128, 128, 1), (94, 0, 1), (94, 7, 1)),
    "eps0 col 130x260 e5m2 f32": ((4909, 442, 52), (4909, 0, 52), (6656, 6656, 52), (4909, 0, 52), (4909, 415, 52)),
    "eps0 full 130x260 e5m2 f32": ((12279, 1103, 2), (12274, 0, 1), (512, 512, 1), (189, 0, 1), (189, 16, 1)),
    "eps0 full 130x257 e5m2 f32": ((12274, 1102, 1), (12274, 0, 1), (128, 128, 1), (189, 0, 1), (189, 16, 1)),
    "eps0 row 3x256 e5m2 bf16": ((4, 0, 2), (94, 0, 1), (128, 128, 1), (2, 0, 1), (2, 0, 1)),
    "eps0 col 130x260 e5m2 bf16": ((104, 0, 52), (4909, 0, 52), (6656, 6656, 52), (104, 0, 52), (104, 0, 52)),
    "eps0 full 130x260 e5m2 bf16": ((256, 0, 2), (12274, 0, 1), (512, 512, 1), (4, 0, 1), (4, 0, 1)),
    "eps0 full 130x257 e5m2 bf16": ((254, 0, 1), (12274, 0, 1), (128, 128, 1), (4, 0, 1), (4, 0, 1)),
    "nt0 row 128x128 e4m3fn f32": ((2455, 212, 26), (2455, 0, 26), (3328, 3328, 26), (2360, 88, 25), (2360, 205, 25)),
    "nt1 row 128x128 e4m3fn f32": ((2360, 204, 25), (2453, 0, 26), (3328, 3328, 26), (2453, 92, 26), (2360, 203, 25)),
    "nt0 col 128x128 e5m2 f32": ((2455, 224, 26), (2455, 0, 26), (3328, 3328, 26), (2361, 0, 25), (2361, 198, 25)),
    "nt1 col 128x128 e5m2 f32": ((2361, 213, 25), (2457, 0, 26), (3328, 3328, 26), (2457, 0, 26), (2361, 198, 25)),
    "nt0 full 128x128 e4m3fn f32": ((12275, 1068, 1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)),
    "nt1 full 128x128 e4m3fn f32": ((0, 0, 0), (12274, 0, 1), (0, 0, 0), (0, 0, 0), (0, 0, 0)),
    "nt0 full 128x128 e5m2 bf16": ((254, 0, 1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)),
    "nt1 full 128x128 e5m2 bf16": ((0, 0, 0), (12275, 0, 1), (0, 0, 0), (0, 0, 0), (0, 0, 0)),
}


def test_the_half_searches_find_what_is_written_here():
    for fmt in FMTS:
        for dtype in ob.HALF:
            got = tuple(ob.half_search(fmt, dtype, m)[1:] for m in ob.tie_ranges(fmt, dtype))
            assert got == SEARCH[f"{_id[fmt]} {_id[dtype]}"], (fmt, dtype, got)
            for k in (0, 3, 4):         # the values that fill the tile: those patterns first, then their neighbours
                v, taken, wrong = ob.half_search(fmt, dtype, ob.tie_ranges(fmt, dtype)[k])
                assert v.numel() == 0 if taken == 0 else v.numel() >= 128
    assert len(SEARCH) == 4


def test_every_input_of_the_gpu_tests_takes_the_redo():
    seen = set()
    for name, x, fmt, tile, dtype, seed in cases():
        seen.add(name)
        got = counts_by_kind(x, fmt, tile, seed)
        assert got == COUNTS[name], f"{name}: {got}"
        ranges = ob.tie_ranges(fmt, dtype)
        # the tiles are what tie_case says: every scale is its kind's range / fmax, bit for bit
        kinds = ob.tie_kind_of_tiles(x.shape, tile, seed)
        scales = ob.oracle(x.float(), fmt, tile, TIE_EPS)[1].view(kinds.shape)
        assert torch.equal(scales, torch.tensor(ranges)[kinds] / FMAX[fmt]), name
        for k, (taken, wrong, tiles) in enumerate(got):
            if not tiles:
                continue
            if dtype == torch.float32:
                can_take, can_be_wrong = True, False        # (which kinds are wrong without the redo: below)
            else:
                can_take, can_be_wrong = (n > 0 for n in SEARCH[f"{_id[fmt]} {_id[dtype]}"][k])
            if not can_take:
                assert (taken, wrong) == (0, 0), f"{name}, {TIE_KINDS[k]}"
                continue
            assert taken >= 1, f"{name}: no element of a {TIE_KINDS[k]} tile takes the redo"
            if can_be_wrong:
                assert wrong >= 1, f"{name}: no element of a {TIE_KINDS[k]} tile is wrong without the redo"
        if dtype == torch.float32 and any(got[k][2] for k in INEXACT):
            assert sum(got[k][1] for k in INEXACT) >= 1, f"{name}: no element of an inexact-scale tile is wrong without the redo"
        if dtype != torch.float16:
            s = scales[kinds == OVERFLOW]
            assert ((s > 0) & (s < 2.0 ** -126)).all() and torch.isinf(1.0 / s).all(), f"{name}: the 1e-37 tiles"
            taken = ob.redo_counts(x, fmt, tile, TIE_EPS)[0]
            tr, tk = tile
            h = torch.clamp(x.shape[0] - tr * torch.arange(kinds.shape[0]), max=tr).view(-1, 1)
            w = torch.clamp(x.shape[1] - tk * torch.arange(kinds.shape[1]), max=tk).view(1, -1)
            assert torch.equal(taken[kinds == OVERFLOW], (h * w)[kinds == OVERFLOW]), f"{name}: all of a 1e-37 tile is divided"
    assert seen == set(COUNTS)


def test_redo_counts_on_the_per_tensor_midpoint_set():
    """the figures the block lane's tests were designed from: one (128, 128) tile holding the whole set under one range"""
    for fmt, n in zip(FMTS, (1009, 985)):
        for m, wrong_e4m3, wrong_e5m2 in ((3.0, 66, 66), (FMAX[fmt] * 2.0 ** -5, 0, 0)):
            s = torch.tensor(m) / FMAX[fmt]
            x = torch.zeros(128, 128)
            V = ob.tie_values(fmt, s)
            assert V.numel() == n
            x.view(-1)[:n] = V
            x[127, 127] = m
            taken, wrong = ob.redo_counts(x, fmt, FULL, TIE_EPS)
            assert int(wrong) == (wrong_e4m3 if fmt == torch.float8_e4m3fn else wrong_e5m2), (fmt, m, int(wrong))
            assert int(taken) == (756 if fmt == torch.float8_e4m3fn else 738), (fmt, m, int(taken))
