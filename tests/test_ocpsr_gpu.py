"""The hardware FP8 lanes' stochastic rounding on the GPU (fp8q_ocpsr_* / fp8q_ocpbsr_* / fp8q_ocpbtsr_*, through seed= /
offset= of the six ops) against the oracle of tests/ocpsr_oracle.py, bit for bit: code bytes and the bit patterns of scales
and values, no element left out, no tolerance.  Every case asserts the kernel it means to reach with the route queries
(ops.chunk_route, ops.ocp_block_route, ops.ocp_block_t_route) before it trusts its shape."""
import pytest
import torch

import mxsr_oracle as sro
import ocpb_oracle as ob
import ocpsr_oracle as oo
from ocpb_oracle import COL, FULL, ROW, same
from ocpsr_oracle import E4M3, E5M2, FMAX, FMTS
from test_ocpsr_host import FREQ, FREQ_SEEDS, freq_check, freq_input

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_id = {E4M3: "e4m3fn", E5M2: "e5m2", torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
SEED, OFFSET = 0x0123456789ABCDEF, 2 ** 35 - 64        # the counter's low word wraps inside every tensor below


def _cuda(t):
    return t.cuda()


# ---- one scale per tensor / per channel ------------------------------------------------------------------------------------
def _pt_input(shape, dtype, mv, gen):
    """seeded normals scaled to the range mv (per row or one number), planted NaN, +-inf, -0 and +-mv; cast to dtype"""
    x = torch.randn(shape, generator=gen)
    m = mv.view(-1, 1) if mv.numel() > 1 else mv
    x = x * m * 0.6
    flat = x.view(-1)
    n = flat.numel()
    for at, v in ((1, float("nan")), (2, float("inf")), (n - 2, -float("inf")), (4, -0.0), (n - 1, 0.0)):
        flat[at] = v
    flat[0], flat[n // 2] = mv.view(-1)[0], -mv.view(-1)[-1]
    return x.to(dtype)


def _ranges(C, per_channel, gen):
    """the kinds of maxval: random (inexact quotients), 1e-37 (1 / scale overflows), 3e38, and -- per channel -- a zero row"""
    n = C if per_channel else 1
    rnd = torch.rand(n, generator=gen) * 3 + 0.1
    out = [("random", rnd), ("1e-37", torch.full((n,), 1e-37)), ("3e38", torch.full((n,), 3e38))]
    if per_channel and C > 1:
        z = rnd.clone()
        z[C // 2] = 0.0
        out.append(("zero row", z))
    return out


PT_SHAPES = {"3x5 rows": ((3, 5), True, 0), "3x5 tensor": ((3, 5), False, 0), "7x147 rows": ((7, 147), True, 0),
             "chunk+groups+tail": ((1, 4096 + 16 + 3), False, 0), "off by one": ((5, 823), True, 1)}


@pytest.mark.parametrize("dtype", DTYPES, ids=[_id[d] for d in DTYPES])
@pytest.mark.parametrize("fmt", FMTS, ids=[_id[f] for f in FMTS])
@pytest.mark.parametrize("name", list(PT_SHAPES))
def test_per_tensor_and_per_channel(name, fmt, dtype):
    from fp8q import ops
    shape, pc, shift = PT_SHAPES[name]
    C, inner = shape[0], shape[1]
    gen = torch.Generator().manual_seed(17)
    for kind, mv in _ranges(C, pc, gen):
        x = _pt_input(shape, dtype, mv, gen)
        if kind == "zero row":
            x[C // 2] = 0.0
            x[C // 2, 0] = -0.0
        base = torch.zeros(x.numel() + 8, dtype=dtype).cuda()
        xd = base[shift:shift + x.numel()].view(shape)
        xd.copy_(x)
        mod = xd.data_ptr() % 16
        route = ops.chunk_route(C, inner, per_channel=pc, in_mod16=mod, out_mod16=0)
        assert route["vec"] == (shift == 0) and not route["nontemporal"], (name, route)
        what = f"{name} {_id[fmt]} {_id[dtype]} maxval {kind}"
        ref_c, ref_s, ref_v = oo.oracle(x.float(), mv, fmt, seed=SEED, offset=OFFSET)
        codes, scale = ops.ocp_encode(xd, _cuda(mv), fmt, seed=SEED, offset=OFFSET)
        same(codes, ref_c, what + ": codes")
        same(scale, ref_s, what + ": scale")
        for out_dtype in ((None,) if dtype == torch.float32 else (None, dtype)):
            y = ops.ocp_quantize(xd, _cuda(mv), fmt, out_dtype=out_dtype, seed=SEED, offset=OFFSET)
            same(y, ref_v if out_dtype is None else ref_v.to(out_dtype), what + f": values as {out_dtype}")
        same(ops.ocp_decode(codes, scale), ref_v, what + ": decode(encode)")


# ---- one scale per tile ----------------------------------------------------------------------------------------------------
# (tile, shape, kernel, dtypes): edge tiles on every vector route; K % 128 != 0 sends row tiles to the plain route; the half
# dtypes where K % 8 == 0
BLOCK_CASES = [(ROW, (130, 256), "rows", DTYPES), (ROW, (130, 260), "plain", (torch.float32,)),
               (COL, (130, 260), "panel", (torch.float32,)), (FULL, (130, 260), "panel", (torch.float32,)),
               (COL, (130, 264), "panel", DTYPES[1:]), (FULL, (130, 264), "panel", DTYPES[1:]),
               (ROW, (129, 131), "plain", DTYPES), (COL, (129, 131), "plain", (torch.float32,)),
               (FULL, (129, 131), "plain", (torch.float32,))]
_block_params = [(t, s, k, d) for t, s, k, ds in BLOCK_CASES for d in ds]


@pytest.mark.parametrize("fmt", FMTS, ids=[_id[f] for f in FMTS])
@pytest.mark.parametrize("tile,shape,kernel,dtype", _block_params,
                         ids=[f"{t[0]}x{t[1]}-{s[0]}x{s[1]}-{k}-{_id[d]}" for t, s, k, d in _block_params])
def test_tile_scaled(tile, shape, kernel, dtype, fmt):
    """ob.case plants, tile by tile, +-0, +-amax, subnormal midpoints, a tile with infinities, a tile of zeros, a NaN tile"""
    from fp8q import ops
    assert ops.ocp_block_route(*shape, tile, dtype) == kernel
    x = ob.case(shape, fmt, tile, seed=3).to(dtype)
    what = f"{tile} {shape} {_id[fmt]} {_id[dtype]} ({kernel})"
    ref_c, ref_s, ref_v = oo.oracle_block(x.float(), fmt, tile, seed=SEED, offset=OFFSET)
    codes, scales = ops.ocp_block_encode(_cuda(x), fmt, tile, seed=SEED, offset=OFFSET)
    same(codes, ref_c, what + ": codes")
    same(scales, ref_s, what + ": scales")
    for out_dtype in ((None,) if dtype == torch.float32 else (None, dtype)):
        y = ops.ocp_block_quantize(_cuda(x), fmt, tile, out_dtype=out_dtype, seed=SEED, offset=OFFSET)
        same(y, ref_v if out_dtype is None else ref_v.to(out_dtype), what + f": values as {out_dtype}")


@pytest.mark.parametrize("tile,shape,kernel", [(ROW, (4, 256), "rows"), (COL, (130, 8), "panel"), (FULL, (130, 132), "panel"),
                                               (FULL, (3, 5), "plain")])
def test_zero_tile_with_eps_zero(tile, shape, kernel):
    """eps = 0: a tile of zeros has scale 0 and q = 0 / 0 -- every code 0x7F whatever the draw; its neighbours are untouched"""
    from fp8q import ops
    assert ops.ocp_block_route(*shape, tile, torch.float32) == kernel
    x = torch.randn(shape, generator=torch.Generator().manual_seed(2))
    x[:tile[0], :tile[1]] = 0.0
    ref_c, ref_s, ref_v = oo.oracle_block(x, E4M3, tile, eps=0.0, seed=7)
    assert (oo.bits(ref_c)[0, 0] == 0x7F) and ref_s.flatten()[0].item() == 0.0
    codes, scales = ops.ocp_block_encode(_cuda(x), E4M3, tile, eps=0.0, seed=7)
    same(codes, ref_c, f"{tile} {shape}: codes")
    same(scales, ref_s, f"{tile} {shape}: scales")
    same(ops.ocp_block_quantize(_cuda(x), E4M3, tile, eps=0.0, seed=7), ref_v, f"{tile} {shape}: values")


# ---- the transposed operands -----------------------------------------------------------------------------------------------
# shape -> (kernel, bytes per store of transposed codes): R % 16 == 0, R % 4 == 0, neither; the plain route
T_SHAPES = {(144, 260): ("panel", 16), (132, 132): ("panel", 4), (130, 260): ("panel", 1), (129, 131): ("plain", 1)}
_t_params = [(s, d) for s in T_SHAPES for d in (DTYPES if s in ((144, 260), (129, 131)) else DTYPES[:1])]


@pytest.mark.parametrize("fmt", FMTS, ids=[_id[f] for f in FMTS])
@pytest.mark.parametrize("tile", [ROW, FULL], ids=["1x128", "128x128"])
@pytest.mark.parametrize("shape,dtype", _t_params, ids=[f"{s[0]}x{s[1]}-{_id[d]}" for s, d in _t_params])
def test_transposed_operands(shape, dtype, tile, fmt):
    from fp8q import ops
    R, K = shape
    kernel, width = T_SHAPES[shape]
    assert ops.ocp_block_t_route(R, K, tile, dtype) == {"kernel": kernel, "code_store_bytes": width, "nontemporal": False}
    x = ob.case(shape, fmt, tile, seed=5).to(dtype)
    what = f"{tile} {shape} {_id[fmt]} {_id[dtype]} ({kernel}, {width})"
    ref_c, ref_s, _ = oo.oracle_block(x.float(), fmt, tile, seed=SEED, offset=OFFSET)
    ref_ct, ref_st, _ = oo.oracle_block_t(x.float(), fmt, tile, seed=SEED, offset=OFFSET)
    ct, st = ops.ocp_block_encode_t(_cuda(x), fmt, tile, seed=SEED, offset=OFFSET)
    same(ct, ref_ct, what + ": encode_t codes_t")
    same(st, ref_st, what + ": encode_t scales_t")
    c, s, ct2, st2 = ops.ocp_block_encode_both(_cuda(x), fmt, tile, seed=SEED, offset=OFFSET)
    same(c, ref_c, what + ": encode_both codes")
    same(s, ref_s, what + ": encode_both scales")
    same(ct2, ref_ct, what + ": encode_both codes_t")
    same(st2, ref_st, what + ": encode_both scales_t")
    if tile == FULL:
        same(ct2, c.t().contiguous(), what + ": codes_t == codes.t()")


# ---- identities, one small shape per lane -----------------------------------------------------------------------------------
def test_identities_per_tensor_lane():
    from fp8q import ops
    x = torch.randn(24, 200, generator=torch.Generator().manual_seed(1)).cuda()
    mv = x.abs().amax(1)
    for fmt in FMTS:
        c, s = ops.ocp_encode(x, mv, fmt, seed=3)
        same(ops.ocp_quantize(x, mv, fmt, seed=3), ops.ocp_decode(c, s), "quantize == decode(encode)")
        # rows 8..15 start at flat index 8 * 200, a multiple of 8: under their own ranges they are the slice of the whole
        cs, _ = ops.ocp_encode(x[8:16].contiguous(), mv[8:16].contiguous(), fmt, seed=3, offset=8 * 200)
        same(cs, c[8:16], "a row slice under its offset")
        assert not torch.equal(oo.bits(ops.ocp_encode(x, mv, fmt, seed=4)[0]), oo.bits(c)), "two seeds"
        c0, s0 = ops.ocp_encode(x, mv, fmt, seed=None)
        c1, s1 = ops.ocp_encode(x, mv, fmt)
        same(c0, c1, "seed=None is the call without it")
        same(c0, oo.oracle(x.cpu(), mv.cpu(), fmt)[0], "seed=None is round to nearest even")
        same(ops.ocp_quantize(x, mv, fmt, seed=None), ops.ocp_quantize(x, mv, fmt), "seed=None, quantize")


@pytest.mark.parametrize("tile", [ROW, COL, FULL], ids=["1x128", "128x1", "128x128"])
def test_identities_tile_lane(tile):
    from fp8q import ops
    x = torch.randn(256, 256, generator=torch.Generator().manual_seed(1)).cuda()
    fmt = E5M2
    assert ops.ocp_block_route(256, 256, tile, torch.float32) == ("rows" if tile == ROW else "panel")
    c, s = ops.ocp_block_encode(x, fmt, tile, seed=3)
    same(ops.ocp_block_quantize(x, fmt, tile, seed=3), ops.ocp_block_decode(c, s, tile), "quantize == decode(encode)")
    # rows 128..255 are whole tiles of every shape and start at flat index 128 * 256, a multiple of 8
    cs, ss = ops.ocp_block_encode(x[128:].contiguous(), fmt, tile, seed=3, offset=128 * 256)
    same(cs, c[128:], "a row slice under its offset")
    assert not torch.equal(oo.bits(ops.ocp_block_encode(x, fmt, tile, seed=4)[0]), oo.bits(c)), "two seeds"
    c0, s0 = ops.ocp_block_encode(x, fmt, tile, seed=None)
    same(c0, ob.oracle(x.cpu(), fmt, tile)[0], "seed=None is round to nearest even")
    same(ops.ocp_block_quantize(x, fmt, tile, seed=None), ops.ocp_block_quantize(x, fmt, tile), "seed=None, quantize")
    if tile != COL:
        ct, st = ops.ocp_block_encode_t(x, fmt, tile, seed=3)
        b = ops.ocp_block_encode_both(x, fmt, tile, seed=3)
        for got, want, what in zip(b, (c, s, ct, st), ("codes", "scales", "codes_t", "scales_t")):
            same(got, want, "encode_both == (encode, encode_t): " + what)
        if tile == FULL:
            same(ct, c.t().contiguous(), "codes_t == codes.t()")
        r = ops.ocp_block_encode_both(x, fmt, tile, seed=None)
        for got, want in zip(r, ops.ocp_block_encode_both(x, fmt, tile)):
            same(got, want, "seed=None is the call without it")


def test_quantizers_draw_seed_by_seed():
    from fp8q import ops
    from quantization.ocp import OCPBlockFP8Quantizer, OCPFP8Quantizer
    x = torch.randn(128, 256, generator=torch.Generator().manual_seed(1)).cuda()
    q = OCPBlockFP8Quantizer(fmt=E5M2, tile=(128, 128), stochastic=True, seed=40)
    with torch.no_grad():
        y0, y1 = q(x), q(x)
        both = q.encode_both(x)
    same(y0, ops.ocp_block_quantize(x, E5M2, (128, 128), seed=40), "call 0")
    same(y1, ops.ocp_block_quantize(x, E5M2, (128, 128), seed=41), "call 1")
    assert q.last_seed == 42
    for got, want in zip(both, ops.ocp_block_encode_both(x, E5M2, (128, 128), seed=42)):
        same(got, want, "call 2")
    p = OCPFP8Quantizer(fmt=E4M3, stochastic=True, seed=7)
    p.set_quant_range(x.min(), x.max())
    with torch.no_grad():
        y = p(x)
    same(y, ops.ocp_quantize(x, p.range_maxval, E4M3, seed=7), "per tensor")


# ---- the nontemporal instantiations (2^24 elements or more), one per kernel ---------------------------------------------------
NT_N = 4112 * 4100
_nt_cache = {}


def _nt_draws(shape):
    """the draws of the largest case, made once: a draw belongs to the flat index, so every shape is a prefix of them"""
    if "r" not in _nt_cache:
        _nt_cache["r"] = sro.draws(SEED, OFFSET, (NT_N,))
    n = shape[0] * shape[1]
    return _nt_cache["r"][:n].view(shape)


def _nt_input(shape):
    if "x" not in _nt_cache:
        g = torch.Generator().manual_seed(9)
        _nt_cache["x"] = torch.randn(NT_N, generator=g)
    n = shape[0] * shape[1]
    x = (_nt_cache["x"][:n].view(shape) * torch.logspace(-3, 3, shape[1])).contiguous()
    x[0, 1], x[1, 0], x[-1, -1], x[-1, -2] = float("nan"), -0.0, float("inf"), 0.0
    return x


def test_nontemporal_per_tensor_encode_and_quantize():
    """k_ocp<encode / quantize, VEC, NT, SR>: float32 [4097, 4099], the last chunk partial with a tail"""
    from fp8q import ops
    shape = (4097, 4099)
    assert ops.chunk_route(*shape, per_channel=True)["nontemporal"] and ops.chunk_route(*shape, per_channel=True)["vec"]
    x, r = _nt_input(shape), _nt_draws(shape)
    mv = torch.nan_to_num(x, nan=0.0, posinf=0.0).abs().amax(1)
    ref_c, ref_s, ref_v = oo.oracle(x, mv, E5M2, r=r)
    c, s = ops.ocp_encode(_cuda(x), _cuda(mv), E5M2, seed=SEED, offset=OFFSET)
    same(c, ref_c, "codes")
    same(s, ref_s, "scale")
    same(ops.ocp_quantize(_cuda(x), _cuda(mv), E5M2, seed=SEED, offset=OFFSET), ref_v, "values")


@pytest.mark.parametrize("tile,shape,kernel,fmt", [(ROW, (4097, 4096), "rows", E4M3), (COL, (4100, 4100), "panel", E5M2),
                                                   (FULL, (4100, 4100), "panel", E4M3)],
                         ids=["rows", "column panels", "full panels"])
def test_nontemporal_tile_scaled(tile, shape, kernel, fmt):
    """k_ocpb_rows<NT, SR>, k_ocpb_panel<kTileCol / kTileFull, NT, SR>, encode and quantize"""
    from fp8q import ops
    assert shape[0] * shape[1] >= 2 ** 24 and ops.ocp_block_route(*shape, tile, torch.float32) == kernel
    assert ops.ocp_block_t_route(*shape, FULL if tile == COL else tile, torch.float32)["nontemporal"]
    x, r = _nt_input(shape), _nt_draws(shape)
    ref_c, ref_s, ref_v = oo.oracle_block(x, fmt, tile, r=r)
    c, s = ops.ocp_block_encode(_cuda(x), fmt, tile, seed=SEED, offset=OFFSET)
    same(c, ref_c, "codes")
    same(s, ref_s, "scales")
    same(ops.ocp_block_quantize(_cuda(x), fmt, tile, seed=SEED, offset=OFFSET), ref_v, "values")


@pytest.mark.parametrize("tile,fmt", [(ROW, E5M2), (FULL, E4M3)], ids=["1x128", "128x128"])
def test_nontemporal_transposed(tile, fmt):
    """k_ocpbt_panel<encode_t / encode_both, NT, SR> at 16-byte stores of the transposed codes"""
    from fp8q import ops
    shape = (4112, 4100)
    assert ops.ocp_block_t_route(*shape, tile, torch.float32) == {"kernel": "panel", "code_store_bytes": 16, "nontemporal": True}
    x, r = _nt_input(shape), _nt_draws(shape)
    ref_c, ref_s, _ = oo.oracle_block(x, fmt, tile, r=r)
    ref_ct, ref_st, _ = oo.oracle_block(x.t().contiguous(), fmt, tile, r=r.t().contiguous())
    ct, st = ops.ocp_block_encode_t(_cuda(x), fmt, tile, seed=SEED, offset=OFFSET)
    same(ct, ref_ct, "encode_t codes_t")
    same(st, ref_st, "encode_t scales_t")
    for got, want, what in zip(ops.ocp_block_encode_both(_cuda(x), fmt, tile, seed=SEED, offset=OFFSET),
                               (ref_c, ref_s, ref_ct, ref_st), ("codes", "scales", "codes_t", "scales_t")):
        same(got, want, "encode_both " + what)


# ---- the frequency of rounding away from zero ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FREQ))
def test_frequency_on_the_kernels(name):
    from fp8q import ops
    from quantization.ocp import OCPFP8Quantizer
    fmt = FREQ[name][0]
    x = freq_input(name)
    mv = torch.tensor([FMAX[fmt]])
    q = OCPFP8Quantizer(fmt=fmt, stochastic=True, seed=FREQ_SEEDS[0])
    q.set_quant_range(-mv, mv)
    ups = []
    for seed in FREQ_SEEDS:
        with torch.no_grad():
            y = q(_cuda(x))
        assert q.last_seed == seed and q.scale.item() == 1.0
        same(y, oo.oracle(x, mv, fmt, seed=seed)[2], f"{name} seed {seed}")
        ups.append(freq_check(y.cpu().flatten(), name, f"{name} seed {seed}"))
    assert not torch.equal(ups[0], ups[1])
    # the codes go the same way, and so does the tile lane where a tile's own amax pins the scale to 1
    c, s = ops.ocp_encode(_cuda(x), _cuda(mv), fmt, seed=FREQ_SEEDS[0])
    assert torch.equal(c.float().cpu() == FREQ[name][3], ups[0].view(x.shape))
