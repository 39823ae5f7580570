"""The redo route of the tile-scaled hardware FP8 lane, its extreme scales, its decode of every byte and its nontemporal
kernels (csrc/fp8q_ocp_block.hip, csrc/fp8q_ocp_block_t.hip, both through csrc/fp8q_ocpq.h) against the oracle of
tests/ocpb_oracle.py, on integers: code bytes and the bit patterns of scales and values, no element left out, no tolerance.

A code is made from x * fl(1/s) and redone by the division x / s where the two ends of the error interval disagree or the
product is NaN; the redo is the only reader of the scale itself in the encoding kernels.  ocpb_oracle.tie_case fills every tile
with rounding ties under the tile's own scale -- under ranges whose reciprocal is exact, inexact, overflowing (a subnormal
scale) and tiny (a huge range) -- so that most elements take the redo; tests/test_ocpb_host.py asserts on the CPU that the
inputs used here do, and how many of them a kernel without the redo would get wrong.  The kernel a case reaches is asserted
beside its comparison."""
import functools
import time

import pytest
import torch

import ocpb_oracle as ob
from ocpb_oracle import COL, FMAX, FMTS, FULL, INT, ROW, TIE_EPS, same

pytestmark = pytest.mark.gpu

_id = {torch.float8_e4m3fn: "e4m3fn", torch.float8_e5m2: "e5m2", torch.float32: "f32", torch.float16: "f16",
       torch.bfloat16: "bf16"}


def _ids(v):
    return _id.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else None)


def _check_lane(x, fmt, tile, what, eps):
    """tests/test_ocpb_gpu.py's assertions: every entry point of the row-wise lane on one tensor (x on the CPU, float32 or
    half) against the oracle of x.float()"""
    from fp8q import ops
    ref_c, ref_s, ref_y = ob.oracle(x.float(), fmt, tile, eps)
    xd = x.cuda()
    codes, scales = ops.ocp_block_encode(xd, fmt, tile, eps=eps)
    assert codes.dtype == fmt and codes.shape == x.shape and scales.dtype == torch.float32
    same(scales, ref_s, f"{what}: scales")
    same(codes, ref_c, f"{what}: codes")
    outs = [torch.float32] if x.dtype == torch.float32 else [torch.float32, x.dtype]
    for dt in outs:
        y = ops.ocp_block_quantize(xd, fmt, tile, eps=eps, out_dtype=dt)
        assert y.dtype == dt and y.shape == x.shape
        same(y, ref_y.to(dt), f"{what}: quantize -> {dt}")
        d = ops.ocp_block_decode(codes, scales, tile, out_dtype=dt)
        # (bit for bit, NaN payloads included: both are this library's)
        assert torch.equal(y.view(INT[dt]), d.view(INT[dt])), f"{what}: quantize != decode(encode) -> {dt}"
    return codes, scales


# ---- the row-wise lane ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ob.TIE_DTYPES, ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile,shape,kernel", ob.TIE_LANE_CASES, ids=_ids)
def test_ties_under_tile_scales(tile, shape, kernel, fmt, dtype):
    from fp8q import ops
    assert ops.ocp_block_route(*shape, tile, dtype) == kernel
    x = ob.tie_case(shape, fmt, tile, dtype)
    _check_lane(x, fmt, tile, f"{tile} {shape} {_id[fmt]} {_id[dtype]} ({kernel})", TIE_EPS)


# ---- the transposed lane ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _t_case(shape, fmt, tile, dtype, transposed_plant):
    """(x on the CPU, the oracle's (codes, scales) of x, those of x.t()), made once and left unchanged"""
    R, K = shape
    x = ob.tie_case((K, R), fmt, tile, dtype).t().contiguous() if transposed_plant else ob.tie_case(shape, fmt, tile, dtype)
    ref = ob.oracle(x.float(), fmt, tile, TIE_EPS)[:2]
    ref_t = ob.oracle(x.float().t().contiguous(), fmt, tile, TIE_EPS)[:2]
    return x, ref, ref_t


@pytest.mark.parametrize("dtype", ob.TIE_DTYPES, ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile", [ROW, FULL], ids=_ids)
@pytest.mark.parametrize("shape", list(ob.TIE_T_SHAPES), ids=_ids)
def test_ties_in_the_transposed_operands(shape, tile, fmt, dtype):
    from fp8q import ops
    R, K = shape
    kernel, width = ob.TIE_T_SHAPES[shape]
    assert ops.ocp_block_t_route(R, K, tile, dtype) == {"kernel": kernel, "code_store_bytes": width, "nontemporal": False}
    for planted in (False, True):
        x, ref, ref_t = _t_case(shape, fmt, tile, dtype, planted)
        what = f"{tile} {shape} {_id[fmt]} {_id[dtype]} ({kernel}, {width}, planted {'transposed' if planted else 'row-wise'})"
        xd = x.cuda()
        ct, st = ops.ocp_block_encode_t(xd, fmt, tile, eps=TIE_EPS)
        assert ct.dtype == fmt and tuple(ct.shape) == (K, R) and st.dtype == torch.float32 and ct.is_contiguous()
        same(st, ref_t[1], f"{what}: encode_t scales_t")
        same(ct, ref_t[0], f"{what}: encode_t codes_t")
        c, s, ct, st = ops.ocp_block_encode_both(xd, fmt, tile, eps=TIE_EPS)
        assert tuple(c.shape) == (R, K) and tuple(ct.shape) == (K, R)
        same(s, ref[1], f"{what}: encode_both scales")
        same(c, ref[0], f"{what}: encode_both codes")
        same(st, ref_t[1], f"{what}: encode_both scales_t")
        same(ct, ref_t[0], f"{what}: encode_both codes_t")
        if tile == FULL:            # one quantization stored twice
            assert torch.equal(ct.view(torch.uint8), c.view(torch.uint8).t()), f"{what}: codes_t != codes.t()"
            assert torch.equal(st.view(torch.int32), s.view(torch.int32).t()), f"{what}: scales_t != scales.t()"


# ---- eps = 0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile,shape,kernel", [(ROW, (3, 256), "rows"), (COL, (130, 260), "panel"), (FULL, (130, 260), "panel"),
                                               (FULL, (130, 257), "plain")], ids=_ids)
def test_eps_zero_a_zero_tile_and_a_subnormal_scale(tile, shape, kernel, fmt, dtype):
    """eps = 0: the tile of zeros has scale 0 and 0 / 0, NaN by the contract -- every code 0x7F, every value NaN; the tile of
    range 1e-37 beside it (tie_case's third) has a subnormal scale whose reciprocal overflows, so all of it is divided"""
    from fp8q import ops
    tr, tk = tile
    assert ops.ocp_block_route(*shape, tile, dtype) == kernel
    x = ob.tie_case(shape, fmt, tile, dtype)
    x[:tr, :tk] = 0.0
    x[0, 0] = -0.0
    codes, scales = _check_lane(x, fmt, tile, f"eps=0 {tile} {shape} {_id[fmt]} {_id[dtype]} ({kernel})", 0.0)
    c, s = codes.view(torch.uint8).cpu(), scales.cpu().flatten()
    assert s[0].view(torch.int32).item() == 0, "the zero tile: scale +0"
    assert (c[:tr, :tk] == 0x7F).all(), "the zero tile: every code 0x7F"
    assert torch.isnan(ops.ocp_block_decode(codes, scales, tile)[:tr, :tk]).all(), "the zero tile decodes to NaN"
    assert ob.tie_kind_of_tiles(shape, tile).flatten()[2].item() == 2
    tiny = s[2].item()
    assert 0.0 < tiny < 2.0 ** -126 and torch.isinf(1.0 / s[2]), "the 1e-37 tile: a subnormal scale, 1 / s overflows"


# ---- decode of every byte ---------------------------------------------------------------------------------------------------
DECODE_SCALES = [1.0, 2.0 ** -7, 3.0 / 448, 1e-6, 1234.5, 0.0, 1e-40, float("inf"), float("nan"), -2.0]


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile", ob.TILES, ids=_ids)
@pytest.mark.parametrize("shape,vec", [((256, 256), True), ((130, 258), False), ((132, 260), True)], ids=_ids)
def test_decode_every_byte_under_every_kind_of_scale(shape, vec, tile, fmt):
    """codes[r, c] = (3 r + c) % 256 -- every row is arange(256) rotated, by 3 a row so that 128 rows of 128 columns hold
    every byte -- under scales drawn per tile, in rotation, from DECODE_SCALES: ordinary ones, 0, a
    subnormal, inf, NaN and a negative one.  Against codes.view(fmt).float() * s on the CPU, into float32, float16 and
    bfloat16; for float32 under finite non-zero scales the exact bits, NaN payloads included.  [256, 256] and [132, 260] take
    the dword kernel (K % 4 == 0, aligned), [130, 258] the element kernel; at [132, 260] the last column group of a (128, 1)
    row reads the four last scales of a ragged K.  With fewer tiles than scales the call is repeated with the rotation
    advanced, so that every (byte, scale) pair is decoded at [256, 256], which is asserted."""
    from fp8q import ops
    R, K = shape
    tr, tk = tile
    nr, nk = -(-R // tr), -(-K // tk)
    codes = ((3 * torch.arange(R).view(R, 1) + torch.arange(K).view(1, K)) % 256).to(torch.uint8)
    cd = codes.cuda()
    assert (K % 4 == 0 and cd.data_ptr() % 16 == 0) == vec         # the launcher's rule for its two decode kernels
    table = torch.tensor(DECODE_SCALES)
    seen = torch.zeros(len(DECODE_SCALES), 256, dtype=torch.bool)
    for first in range(0, len(DECODE_SCALES), min(nr * nk, len(DECODE_SCALES))):
        pick = (torch.arange(nr * nk).view(nr, nk) + first) % len(DECODE_SCALES)
        scales = table[pick]
        full = scales.repeat_interleave(tr, 0).repeat_interleave(tk, 1)[:R, :K]
        seen[pick.repeat_interleave(tr, 0).repeat_interleave(tk, 1)[:R, :K].flatten(), codes.flatten().long()] = True
        ref = codes.view(fmt).float() * full
        sd = scales.cuda()
        what = f"{tile} {shape} {_id[fmt]} rotation {first}"
        got = ops.ocp_block_decode(cd.view(fmt), sd, tile)
        assert got.dtype == torch.float32 and got.shape == codes.shape
        same(got, ref, f"{what}: float32")
        exact = torch.isfinite(full) & (full != 0)
        assert torch.equal(got.cpu().view(torch.int32)[exact], ref.view(torch.int32)[exact]), f"{what}: float32, exact bits"
        assert torch.equal(ops.ocp_block_decode(cd, sd, tile, fmt=fmt).view(torch.int32), got.view(torch.int32)), what
        for dt in (torch.float16, torch.bfloat16):
            same(ops.ocp_block_decode(cd.view(fmt), sd, tile, out_dtype=dt), ref.to(dt), f"{what}: {dt}")
    if shape == (256, 256):
        assert seen.all(), "a (byte, scale) pair was never decoded"


# ---- the nontemporal kernels (2^24 elements or more) against the CPU cast -----------------------------------------------------
def _nt_case(shape, fmt, tile, dtype):
    """seeded normals times a per-column logspace; the first, a middle and the last (edge) panel of 128 x 128 filled by
    tie_case (their tiles begin on the tensor's own tile grid), each from another point of the rotation of ranges; NaN, +-inf,
    -0.0 and 1e-45 planted, and one tile of zeros"""
    R, K = shape
    tr, tk = tile
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(R, K, generator=g) * torch.logspace(-4, 4, K)).to(dtype)
    nR, nK = -(-R // 128), -(-K // 128)
    for n, (pr, pc) in enumerate(((0, 0), (nR // 2, nK // 2), (nR - 1, nK - 1))):
        r = x[128 * pr:128 * (pr + 1), 128 * pc:128 * (pc + 1)]
        r.copy_(ob.tie_case(tuple(r.shape), fmt, tile, dtype, seed=n))
    x[256:256 + tr, 512:512 + tk] = 0.0
    x[300, 5], x[301, 700], x[302, 900], x[R - 1, 0], x[1000, 129] = float("nan"), float("inf"), -float("inf"), -0.0, 1e-45
    return x


def _check_nt(shape, fmt, tile, dtype, kernel, decode_into=()):
    from fp8q import ops
    R, K = shape
    assert R * K >= 2 ** 24
    assert ops.ocp_block_route(R, K, tile, dtype) == kernel
    # (the lane's one size rule, reported by the transposed lane's route query, which has no (128, 1))
    assert ops.ocp_block_t_route(R, K, FULL if tile == COL else tile, dtype)["nontemporal"]
    x = _nt_case(shape, fmt, tile, dtype)
    t0 = time.perf_counter()
    ref_c, ref_s, ref_y = ob.oracle(x.float(), fmt, tile, TIE_EPS)
    t1 = time.perf_counter()
    xd = x.cuda()
    codes, scales = ops.ocp_block_encode(xd, fmt, tile, eps=TIE_EPS)
    same(scales, ref_s, "scales")
    assert torch.equal(codes.view(torch.uint8).cpu(), ref_c.view(torch.uint8)), "codes"
    y = ops.ocp_block_quantize(xd, fmt, tile, eps=TIE_EPS)
    d = ops.ocp_block_decode(codes, scales, tile)
    assert torch.equal(y.view(torch.int32), d.view(torch.int32)), "quantize != decode(encode)"
    same(y, ref_y, "quantize")
    del y, d
    for dt in decode_into:
        y = ops.ocp_block_quantize(xd, fmt, tile, eps=TIE_EPS, out_dtype=dt)
        d = ops.ocp_block_decode(codes, scales, tile, out_dtype=dt)
        assert torch.equal(y.view(INT[dt]), d.view(INT[dt])), f"quantize != decode(encode) -> {dt}"
        same(d, ref_y.to(dt), f"decode -> {dt}")
    torch.cuda.synchronize()
    print(f"nontemporal {tile} {shape} {_id[fmt]} {_id[dtype]}: oracle {t1 - t0:.2f} s, the rest {time.perf_counter() - t1:.2f} s")


def test_nontemporal_rows_against_the_cpu_cast():
    """k_ocpb_rows<NT>, k_ocpb_decode<VEC, NT>: float32 [4097, 4096], 16.78 M elements, the last block partial"""
    _check_nt((4097, 4096), torch.float8_e4m3fn, ROW, torch.float32, "rows")


def test_nontemporal_column_panels_against_the_cpu_cast():
    """k_ocpb_panel<kTileCol, NT>: float32 [4100, 4100], 16.81 M elements, ragged both ways"""
    _check_nt((4100, 4100), torch.float8_e5m2, COL, torch.float32, "panel")


def test_nontemporal_full_panels_against_the_cpu_cast():
    """k_ocpb_panel<kTileFull, NT>: float32 [4100, 4100]"""
    _check_nt((4100, 4100), torch.float8_e4m3fn, FULL, torch.float32, "panel")


def test_nontemporal_full_panels_of_bfloat16_against_the_cpu_cast():
    """k_ocpb_panel<kTileFull, NT> on bfloat16 [4100, 4104], and k_ocpb_decode<VEC, NT> into bfloat16"""
    _check_nt((4100, 4104), torch.float8_e5m2, FULL, torch.bfloat16, "panel", decode_into=(torch.bfloat16,))
