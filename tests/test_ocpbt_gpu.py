"""The transposed operands of the tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block_t.hip: ops.ocp_block_encode_t /
ocp_block_encode_both, OCPBlockFP8Quantizer.encode_t / encode_both) against the oracle of tests/ocpb_oracle.py and against the
merged row-wise kernels, on integers: code bytes and the bit patterns of the float32 scales, no element left out.  The oracle
of the transposed operands of x is the oracle of the contiguous x.t(); the route a case reaches is asserted beside its
comparison.  Inputs come two ways: ocpb_oracle.case of the shape itself (special values at the start of row-wise tiles) and
the transpose of the case of the transposed shape (special values at the start of the transposed tiles)."""
import functools

import pytest
import torch

import ocpb_oracle as ob
from ocpb_oracle import EPS, FMAX, FMTS, same

pytestmark = pytest.mark.gpu

ROW, COL, FULL = (1, 128), (128, 1), (128, 128)
TILES = (ROW, FULL)
# shape -> (kernel, bytes per store of transposed codes) of an aligned tensor: the smallest shapes that reach each branch
SHAPES = {(1, 1): ("plain", 1), (127, 5): ("plain", 1), (129, 131): ("plain", 1), (128, 128): ("panel", 16),
          (256, 384): ("panel", 16), (144, 260): ("panel", 16), (132, 132): ("panel", 4), (130, 260): ("panel", 1),
          (5, 132): ("panel", 1)}
_id = {torch.float8_e4m3fn: "e4m3fn", torch.float8_e5m2: "e5m2", torch.float32: "f32", torch.float16: "f16",
       torch.bfloat16: "bf16"}


def _ids(v):
    return _id.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else None)


@functools.lru_cache(maxsize=None)
def _case(shape, fmt, tile, dtype, transposed_plant, eps=EPS):
    """(x on the CPU, the oracle's (codes, scales) of x, the oracle's (codes, scales) of x.t()), made once and left unchanged"""
    R, K = shape
    x = ob.case((K, R), fmt, tile).t().contiguous() if transposed_plant else ob.case(shape, fmt, tile)
    x = x.to(dtype)
    ref = ob.oracle(x.float(), fmt, tile, eps)[:2]
    ref_t = ob.oracle(x.float().t().contiguous(), fmt, tile, eps)[:2]
    return x, ref, ref_t


def _check(x, ref, ref_t, fmt, tile, what, eps=EPS):
    """encode_t and encode_both of x (on the CPU) against the two oracles; returns encode_both's results"""
    from fp8q import ops
    R, K = x.shape
    xd = x.cuda()
    ct, st = ops.ocp_block_encode_t(xd, fmt, tile, eps=eps)
    assert ct.dtype == fmt and tuple(ct.shape) == (K, R) and st.dtype == torch.float32 and ct.is_contiguous()
    same(st, ref_t[1], f"{what}: encode_t scales_t")
    same(ct, ref_t[0], f"{what}: encode_t codes_t")
    c, s, ct2, st2 = ops.ocp_block_encode_both(xd, fmt, tile, eps=eps)
    assert c.dtype == fmt and tuple(c.shape) == (R, K) and tuple(ct2.shape) == (K, R) and s.dtype == torch.float32
    same(s, ref[1], f"{what}: encode_both scales")
    same(c, ref[0], f"{what}: encode_both codes")
    same(st2, ref_t[1], f"{what}: encode_both scales_t")
    same(ct2, ref_t[0], f"{what}: encode_both codes_t")
    return c, s, ct2, st2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile", TILES, ids=_ids)
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_both_ops_against_the_cpu_cast(shape, tile, fmt, dtype):
    from fp8q import ops
    kernel, width = SHAPES[shape]
    route = ops.ocp_block_t_route(*shape, tile, dtype)
    assert (route["kernel"], route["code_store_bytes"], route["nontemporal"]) == (kernel, width, False)
    for planted in (False, True):
        x, ref, ref_t = _case(shape, fmt, tile, dtype, planted)
        what = f"{tile} {shape} {_id[fmt]} {_id[dtype]} ({kernel}, {width}, planted {'transposed' if planted else 'row-wise'})"
        c, s, ct, st = _check(x, ref, ref_t, fmt, tile, what)
        if tile == FULL:            # one quantization stored twice
            assert torch.equal(ct.view(torch.uint8), c.view(torch.uint8).t())
            assert torch.equal(st.view(torch.int32), s.view(torch.int32).t())
        # the contract's consequences where the case planted them in the transposed tiles (ocpb_oracle.case): a zero tile and
        # a NaN tile where the transposed operands have more than four tiles
        if planted and st.numel() > 4:
            sf = st.cpu().flatten()
            assert sf[1].item() == (torch.tensor(EPS) / FMAX[fmt]).item(), "a zero tile: scale = eps / fmax"
            assert torch.isnan(sf[2]), "a NaN tile: NaN scale"


def test_every_route_that_exists_is_reached():
    from fp8q import ops
    reached = set()
    for shape in SHAPES:
        for tile in TILES:
            for dt in (torch.float32, torch.float16, torch.bfloat16):
                r = ops.ocp_block_t_route(*shape, tile, dt)
                assert (r["kernel"], r["code_store_bytes"]) == SHAPES[shape]
                reached.add((r["kernel"], r["code_store_bytes"]))
    assert reached == {("plain", 1), ("panel", 16), ("panel", 4), ("panel", 1)}


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("shape", [(130, 260), (144, 260), (256, 384)], ids=_ids)
def test_identities_against_the_merged_kernels(shape, fmt):
    """on the GPU, against ocp_block_encode / ocp_block_decode / ocp_block_quantize as they are"""
    from fp8q import ops
    u8, i32 = torch.uint8, torch.int32
    for planted in (False, True):
        for tile in TILES:
            x = _case(shape, fmt, tile, torch.float32, planted)[0].cuda()
            ct, st = ops.ocp_block_encode_t(x, fmt, tile)
            rc, rs = ops.ocp_block_encode(x.t().contiguous(), fmt, tile)
            assert torch.equal(ct.view(u8), rc.view(u8)) and torch.equal(st.view(i32), rs.view(i32)), (tile, planted)
            c, s, ct2, st2 = ops.ocp_block_encode_both(x, fmt, tile)
            c1, s1 = ops.ocp_block_encode(x, fmt, tile)
            assert torch.equal(c.view(u8), c1.view(u8)) and torch.equal(s.view(i32), s1.view(i32)), (tile, planted)
            assert torch.equal(ct2.view(u8), ct.view(u8)) and torch.equal(st2.view(i32), st.view(i32)), (tile, planted)
            if tile == ROW:
                cc, sc = ops.ocp_block_encode(x, fmt, COL)             # the same scales, the codes untransposed
                assert torch.equal(ct.view(u8), cc.view(u8).t()) and torch.equal(st.view(i32), sc.view(i32).t())
                y = ops.ocp_block_decode(ct, st, ROW).t()
                q = ops.ocp_block_quantize(x, fmt, COL)
                assert torch.equal(y.contiguous().view(i32), q.view(i32)), planted       # NaN payloads included: both are ours
            else:
                assert torch.equal(ct.view(u8), c.view(u8).t()) and torch.equal(st.view(i32), s.view(i32).t())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("tile", TILES, ids=_ids)
def test_a_view_offset_by_one_element_takes_the_plain_route_with_identical_bytes(tile, dtype):
    from fp8q import ops
    fmt, shape = torch.float8_e4m3fn, (130, 260)
    x, ref, ref_t = _case(shape, fmt, tile, dtype, True)
    n = x.numel()
    xd = torch.zeros(n + 1, dtype=dtype, device="cuda")[1:]
    xd.copy_(x.flatten())
    xd = xd.view(shape)
    assert xd.data_ptr() % 16 != 0 and xd.is_contiguous()
    assert ops.ocp_block_t_route(*shape, tile, dtype, aligned16=False)["kernel"] == "plain"
    assert ops.ocp_block_t_route(*shape, tile, dtype)["kernel"] == "panel"
    ct, st = ops.ocp_block_encode_t(xd, fmt, tile)
    same(st, ref_t[1], "scales_t")
    same(ct, ref_t[0], "codes_t")
    slow = ops.ocp_block_encode_both(xd, fmt, tile)
    fast = ops.ocp_block_encode_both(x.cuda(), fmt, tile)
    for a, b, r, name in zip(slow, fast, (ref[0], ref[1], ref_t[0], ref_t[1]), ("codes", "scales", "codes_t", "scales_t")):
        same(a, r, name)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name


@pytest.mark.parametrize("tile", TILES, ids=_ids)
@pytest.mark.parametrize("shape", [(144, 260), (130, 260), (132, 132)], ids=_ids)
def test_outputs_in_place_leave_their_guard_bytes(shape, tile):
    """every output in the middle of a larger buffer, 64 bytes of 0xA5 on each side (the 16-byte alignment stays): the wide
    transposed stores at ragged edges write nothing outside their tensor, and the returned tensors are the buffers"""
    from fp8q import ops
    fmt, G = torch.float8_e4m3fn, 64
    R, K = shape
    x, ref, ref_t = _case(shape, fmt, tile, torch.float32, True)
    xd = x.cuda()
    assert ops.ocp_block_t_route(R, K, tile, torch.float32) == {"kernel": "panel", "code_store_bytes": SHAPES[shape][1],
                                                               "nontemporal": False}

    def guarded(nbytes):
        return torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")

    def intact(buf, what):
        assert (buf[:G] == 0xA5).all() and (buf[-G:] == 0xA5).all(), f"{what}: guard bytes overwritten"

    n = R * K
    bc, bct = guarded(n), guarded(n)
    bs, bst = guarded(4 * ref[1].numel()), guarded(4 * ref_t[1].numel())
    out, out_t = bc[G:G + n], bct[G:G + n].view(fmt)
    s_out = bs[G:-G].view(torch.float32).view(ref[1].shape)
    st_out = bst[G:-G].view(torch.float32).view(ref_t[1].shape)
    for t in (out, out_t, s_out, st_out):
        assert t.data_ptr() % 16 == 0
    ct, st = ops.ocp_block_encode_t(xd, fmt, tile, out=out_t, scales_out=st_out)
    assert ct.data_ptr() == out_t.data_ptr() and st.data_ptr() == st_out.data_ptr()
    same(ct, ref_t[0], "encode_t codes_t")
    same(st, ref_t[1], "encode_t scales_t")
    intact(bct, "encode_t codes_t")
    intact(bst, "encode_t scales_t")
    bct[G:-G] = 0xA5
    bst[G:-G] = 0xA5
    c, s, ct, st = ops.ocp_block_encode_both(xd, fmt, tile, out=out, scales_out=s_out, out_t=out_t, scales_out_t=st_out)
    assert c.data_ptr() == out.data_ptr() and s.data_ptr() == s_out.data_ptr()
    assert ct.data_ptr() == out_t.data_ptr() and st.data_ptr() == st_out.data_ptr()
    for got, want, buf, name in ((c, ref[0], bc, "codes"), (s, ref[1], bs, "scales"), (ct, ref_t[0], bct, "codes_t"),
                                 (st, ref_t[1], bst, "scales_t")):
        same(got, want, f"encode_both {name}")
        intact(buf, f"encode_both {name}")


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile", TILES, ids=_ids)
def test_a_non_default_eps_sets_the_scale_of_the_zero_tile(tile, fmt):
    eps, shape = 1e-3, (130, 260)
    for planted in (False, True):
        x, ref, ref_t = _case(shape, fmt, tile, torch.float32, planted, eps)
        c, s, ct, st = _check(x, ref, ref_t, fmt, tile, f"eps {tile} {_id[fmt]} planted {planted}", eps=eps)
        zero = (st if planted else s).cpu().flatten()[1]              # ocpb_oracle.case: tile 1 is the tile of zeros
        assert zero.item() == (torch.tensor(eps, dtype=torch.float32) / FMAX[fmt]).item()
        assert zero.item() != (torch.tensor(EPS) / FMAX[fmt]).item()


def test_the_nontemporal_regime():
    """float32 [4112, 4096]: 64.25 MiB of values, so the panel kernels take their nontemporal variants; 4112 = 32 x 128 + 16
    leaves a short last panel.  Compared on the GPU with the merged row-wise kernels."""
    from fp8q import ops
    fmt, (R, K) = torch.float8_e4m3fn, (4112, 4096)
    u8, i32 = torch.uint8, torch.int32
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(R, K, device="cuda", generator=g) * torch.logspace(-4, 4, K, device="cuda")
    x[0, 0], x[200, 300], x[4111, 4095], x[1000, 129] = float("inf"), float("nan"), -0.0, 1e-45
    x[256:384, 512:640] = 0.0
    xt = x.t().contiguous()
    for tile in TILES:
        route = ops.ocp_block_t_route(R, K, tile, torch.float32)
        assert route == {"kernel": "panel", "code_store_bytes": 16, "nontemporal": True}
        rc, rs = ops.ocp_block_encode(x, fmt, tile)
        rct, rst = ops.ocp_block_encode(xt, fmt, tile)
        ct, st = ops.ocp_block_encode_t(x, fmt, tile)
        assert torch.equal(ct.view(u8), rct.view(u8)) and torch.equal(st.view(i32), rst.view(i32)), tile
        del ct, st
        c, s, ct, st = ops.ocp_block_encode_both(x, fmt, tile)
        assert torch.equal(c.view(u8), rc.view(u8)) and torch.equal(s.view(i32), rs.view(i32)), tile
        assert torch.equal(ct.view(u8), rct.view(u8)) and torch.equal(st.view(i32), rst.view(i32)), tile
        del c, s, ct, st, rc, rs, rct, rst


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile", TILES, ids=_ids)
def test_quantizer_encode_t_and_encode_both(tile, fmt):
    from fp8q import ops
    from quantization.ocp import OCPBlockFP8Quantizer as Q
    u8, i32 = torch.uint8, torch.int32
    eps = 1e-6
    g = torch.Generator().manual_seed(1)
    for w in (torch.randn(136, 256, generator=g).cuda(), torch.randn(8, 3, 3, 3, generator=g).cuda().bfloat16()):
        q = Q(fmt=fmt, tile=tile, eps=eps, flatten_rows=True)
        w2 = w.view(w.shape[0], -1)
        want_t = ops.ocp_block_encode_t(w2, fmt, tile, eps=eps)
        want = ops.ocp_block_encode_both(w2, fmt, tile, eps=eps)
        ref = ob.oracle(w2.float().cpu().t().contiguous(), fmt, tile, eps)
        same(want_t[0], ref[0], "codes_t")
        same(want_t[1], ref[1], "scales_t")
        got_t = q.encode_t(w)
        got = q.encode_both(w)
        assert tuple(got_t[0].shape) == (w2.shape[1], w2.shape[0]) and got_t[0].dtype == fmt
        for a, b in zip(got_t + got, want_t + want):
            assert a.shape == b.shape and a.dtype == b.dtype
            assert torch.equal(a.view(u8), b.view(u8))
        enc = q.encode(w)
        assert torch.equal(got[0].view(u8), enc[0].view(u8)) and torch.equal(got[1].view(i32), enc[1].view(i32))
        if tile == ROW:
            y = q.decode(*got_t).t().contiguous()
            f = Q(fmt=fmt, tile=COL, eps=eps, flatten_rows=True)(w).view(w2.shape)
            assert torch.equal(y.view(i32), f.contiguous().view(i32))
