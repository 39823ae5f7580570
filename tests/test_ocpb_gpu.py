"""The tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block.hip: ops.ocp_block_encode / ocp_block_decode / ocp_block_quantize,
OCPBlockFP8Quantizer) against the oracle of tests/ocpb_oracle.py -- torch's CPU cast under scales taken per 1x128, 128x1 or
128x128 tile -- on integers: code bytes, and the bit patterns of scales and of float32 / float16 / bfloat16 values.  No element
is left out of any comparison; NaNs are mapped to one pattern where values are compared and stored as 0x7F in the oracle's
codes (tests/ocpb_oracle.py says why).  The kernel a case reaches is asserted beside its comparison."""
import pytest
import torch

import ocpb_oracle as ob
from ocpb_oracle import EPS, FMAX, FMTS, INT, same

pytestmark = pytest.mark.gpu

ROW, COL, FULL = (1, 128), (128, 1), (128, 128)
# shape -> the kernel of an aligned float32 / half tensor.  Rows: the issue's shapes and (40, 256) (more than one block's 32
# tiles); spanning tiles: the issue's and two ragged panels with K % 4 == 0, (5, 132) and (130, 260)
ROW_SHAPES = {(1, 1): "plain", (3, 127): "plain", (5, 128): "rows", (2, 129): "plain", (7, 384): "rows", (2, 3, 260): "plain",
              (40, 256): "rows"}
SPAN_SHAPES = {(1, 1): "plain", (127, 5): "plain", (128, 128): "panel", (129, 131): "plain", (130, 257): "plain",
               (256, 384): "panel", (5, 132): "panel", (130, 260): "panel"}
CASES = [(ROW, s) for s in ROW_SHAPES] + [(t, s) for t in (COL, FULL) for s in SPAN_SHAPES]
_id = {torch.float8_e4m3fn: "e4m3fn", torch.float8_e5m2: "e5m2", torch.float32: "f32", torch.float16: "f16",
       torch.bfloat16: "bf16"}


def _ids(v):
    return _id.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else None)


def _route(shape, tile, dtype, aligned16=True):
    from fp8q import ops
    R = 1
    for s in shape[:-1]:
        R *= s
    return ops.ocp_block_route(R, shape[-1], tile, dtype, aligned16)


def _check_lane(x, fmt, tile, what, eps=EPS):
    """every entry point on one tensor (x on the CPU, float32 or half) against the oracle of x.float()"""
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


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile,shape", CASES, ids=_ids)
def test_codes_scales_and_values_against_the_cpu_cast(tile, shape, fmt, dtype):
    want = (ROW_SHAPES if tile == ROW else SPAN_SHAPES)[shape]
    assert _route(shape, tile, dtype) == want
    x = ob.case(shape, fmt, tile).to(dtype)
    codes, scales = _check_lane(x, fmt, tile, f"{tile} {shape} {_id[fmt]} {_id[dtype]} ({want})")
    # the contract's consequences, where the case planted them (ocpb_oracle.case): the shapes with more than four tiles
    c, s = codes.view(torch.uint8).cpu().view(-1, shape[-1]), scales.cpu().view(-1, scales.shape[-1])
    nk = s.shape[1]
    if s.numel() > 4:
        tr, tk = tile
        t = lambda n: (slice((n // nk) * tr, (n // nk + 1) * tr), slice((n % nk) * tk, (n % nk + 1) * tk))
        assert s.flatten()[1].item() == (torch.tensor(EPS) / FMAX[fmt]).item(), "a zero tile: scale = eps / fmax"
        assert (c[t(1)] & 0x7F == 0).all(), "a zero tile has zero codes"
        assert torch.isnan(s.flatten()[2]) and (c[t(2)] == 0x7F).all(), "a NaN tile: NaN scale, every code 0x7F"
        mid = s.numel() // 2
        if mid > 2 and c[t(mid)].numel() > 1:          # (a one-element edge tile has no room for the planted infinity)
            assert torch.isinf(s.flatten()[mid]), "an infinity in the tile: scale = inf"
            assert ((c[t(mid)] & 0x7F == 0) | (c[t(mid)] == 0x7F)).all()


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_routes_differ_between_aligned_and_ragged_and_are_all_reached(fmt):
    """every tile has two kernels, the route query tells them apart, and the cases above reach each of them"""
    for dt in (torch.float32, torch.bfloat16):
        assert _route((7, 384), ROW, dt) == "rows" and _route((7, 385), ROW, dt) == "plain"
        assert _route((7, 384), ROW, dt, aligned16=False) == "plain"
        for tile in (COL, FULL):
            assert _route((256, 384), tile, dt) == "panel" and _route((256, 383), tile, dt) == "plain"
            assert _route((130, 260), tile, dt) == "panel"
            assert _route((256, 384), tile, dt, aligned16=False) == "plain"
    assert set(ROW_SHAPES.values()) == {"rows", "plain"} and set(SPAN_SHAPES.values()) == {"panel", "plain"}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("tile,shape", [(ROW, (7, 384)), (COL, (256, 384)), (FULL, (256, 384))], ids=_ids)
def test_a_view_offset_by_one_element_takes_the_plain_route_with_identical_bytes(tile, shape, dtype):
    from fp8q import ops
    fmt = torch.float8_e4m3fn
    x = ob.case(shape, fmt, tile).to(dtype)
    n = x.numel()
    xd = torch.zeros(n + 1, dtype=dtype, device="cuda")[1:]
    xd.copy_(x.flatten())
    xd = xd.view(shape)
    assert xd.data_ptr() % 16 != 0 and xd.is_contiguous()
    assert _route(shape, tile, dtype, aligned16=False) == "plain" and _route(shape, tile, dtype) != "plain"
    ref_c, ref_s, ref_y = ob.oracle(x.float(), fmt, tile)
    cbuf = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    codes, scales = ops.ocp_block_encode(xd, fmt, tile, out=cbuf[1:])
    same(codes, ref_c, "codes")
    same(scales, ref_s, "scales")
    assert cbuf[0].item() == 0
    fast_c, fast_s = ops.ocp_block_encode(x.cuda(), fmt, tile)
    assert torch.equal(fast_c.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(fast_s.view(torch.int32),
                                                                                         scales.view(torch.int32))
    ybuf = torch.zeros(n + 1, dtype=dtype, device="cuda")
    y = ops.ocp_block_quantize(xd, fmt, tile, out=ybuf[1:].view(shape))
    same(y, ref_y.to(dtype), "quantize")
    dbuf = torch.zeros(n + 1, dtype=dtype, device="cuda")
    d = ops.ocp_block_decode(codes, scales, tile, out=dbuf[1:].view(shape))
    assert torch.equal(y.view(INT[dtype]), d.view(INT[dtype]))
    assert ybuf[0].item() == 0 and dbuf[0].item() == 0


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("tile,shape", [(ROW, (7, 384)), (ROW, (2, 129)), (COL, (130, 260)), (COL, (129, 131)),
                                        (FULL, (130, 260)), (FULL, (130, 257))], ids=_ids)
def test_a_tile_equals_the_per_tensor_lane_on_that_tile(tile, shape, fmt):
    """ocp_block_encode(x)[tile] == ops.ocp_encode(x[tile].contiguous(), amax, fmt) and its scale_out, on the GPU"""
    from fp8q import ops
    tr, tk = tile
    x = ob.case(shape, fmt, tile).cuda()
    codes, scales = ops.ocp_block_encode(x, fmt, tile)
    nr, nk = scales.shape
    picks = {(0, 0), (nr - 1, nk - 1), (nr // 2, nk // 2), (0, nk - 1), (min(1, nr - 1), 0)}
    for i, j in sorted(picks):
        sub = x[i * tr:(i + 1) * tr, j * tk:(j + 1) * tk].contiguous()
        amax = sub.abs().amax().reshape(1)
        c1, s1 = ops.ocp_encode(sub, amax, fmt, eps=EPS)
        got = codes[i * tr:(i + 1) * tr, j * tk:(j + 1) * tk].contiguous()
        assert torch.equal(got.view(torch.uint8), c1.view(torch.uint8)), (i, j)
        same(scales[i, j].reshape(1), s1, f"scale of tile {(i, j)}")


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("shape", [(130, 260), (129, 131), (256, 384)], ids=_ids)
def test_orientation_identities(shape, fmt):
    """(128, 1) of x is (1, 128) of x.t().contiguous(), transposed, codes and scales; (128, 128) commutes with the transpose"""
    from fp8q import ops
    x = ob.case(shape, fmt, COL).cuda()
    xt = x.t().contiguous()
    c, s = ops.ocp_block_encode(x, fmt, COL)
    ct, st = ops.ocp_block_encode(xt, fmt, ROW)
    assert torch.equal(c.view(torch.uint8), ct.view(torch.uint8).t()) and same(s, st.t().contiguous(), "scales") is None
    c, s = ops.ocp_block_encode(x, fmt, FULL)
    ct, st = ops.ocp_block_encode(xt, fmt, FULL)
    assert torch.equal(c.view(torch.uint8), ct.view(torch.uint8).t()) and same(s, st.t().contiguous(), "scales") is None
    y, yt = ops.ocp_block_quantize(x, fmt, COL), ops.ocp_block_quantize(xt, fmt, ROW)
    same(y, yt.t().contiguous(), "quantize")


def test_outputs_are_written_in_place_and_eps_is_honoured():
    from fp8q import ops
    fmt = torch.float8_e4m3fn
    x = ob.case((130, 260), fmt, FULL).cuda()
    for tile in ob.TILES:
        ref_c, ref_s = ops.ocp_block_encode(x, fmt, tile)
        out = torch.zeros(130, 260, dtype=torch.uint8, device="cuda")
        so = torch.zeros_like(ref_s)
        c, s = ops.ocp_block_encode(x, fmt, tile, out=out, scales_out=so)
        assert c.data_ptr() == out.data_ptr() and s.data_ptr() == so.data_ptr()
        assert torch.equal(out, ref_c.view(torch.uint8)) and torch.equal(so.view(torch.int32), ref_s.view(torch.int32))
        out8 = torch.zeros(130, 260, dtype=fmt, device="cuda")
        assert ops.ocp_block_encode(x, fmt, tile, out=out8)[0].data_ptr() == out8.data_ptr()
        assert torch.equal(out8.view(torch.uint8), out)
        y = torch.zeros(130, 260, device="cuda")
        assert ops.ocp_block_quantize(x, fmt, tile, out=y).data_ptr() == y.data_ptr()
        d = torch.zeros(130, 260, device="cuda")
        assert ops.ocp_block_decode(c, s, tile, out=d).data_ptr() == d.data_ptr()
        assert torch.equal(y.view(torch.int32), d.view(torch.int32)) and y.abs().nan_to_num().sum().item() > 0
        # a non-default eps on a zero tile (tile 1 of the case), against the oracle and as a number
        for eps in (1e-3, 0.5):
            ce, se = _check_lane(x.cpu(), fmt, tile, f"eps={eps} {tile}", eps=eps)
            if tile != COL:        # (the case's zero tile, rows 0..127 x columns 128..255, is tile 1 of the other two)
                assert se.flatten()[1].item() == (torch.tensor(eps) / 448.0).item()


# ---- quantizer, manager ----------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(256, 136)
        self.conv = torch.nn.Conv2d(3, 8, 3)

    def forward(self, x):                     # [N, 3, 8, 256] -> [N, 3, 8, 136] -> [N, 8, 6, 134]
        return self.conv(torch.relu(self.fc(x)))


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_quantizer_in_a_two_layer_net(fmt):
    from quantization.estimators import RangeEstimators
    from quantization.layers import QuantizedModule, quantize_model
    from quantization.ocp import OCPBlockFP8Quantizer
    torch.manual_seed(0)
    net = quantize_model(_Net(), method=OCPBlockFP8Quantizer, act_method=OCPBlockFP8Quantizer, n_bits=8, n_bits_act=8,
                         per_channel_weights=True, weight_range_method=RangeEstimators.current_minmax.cls,
                         act_range_method=RangeEstimators.running_minmax.cls, fp8_kwargs=dict(fmt=fmt),
                         weight_quant_kwargs=dict(tile=FULL, flatten_rows=True),
                         act_quant_kwargs=dict(tile=ROW)).cuda().eval()
    layers = [m for m in net.modules() if isinstance(m, QuantizedModule)]
    assert len(layers) == 2
    for m in layers:
        m.quantized()
        m.estimate_ranges()
    qs = [m for m in net.modules() if isinstance(m, OCPBlockFP8Quantizer)]
    wq = [net.fc.weight_quantizer.quantizer, net.conv.weight_quantizer.quantizer]
    assert len(qs) == 4 and all(q.fmt == fmt for q in qs)
    assert all(q.tile == FULL and q.flatten_rows for q in wq) and all(q.tile == ROW for q in qs if q not in wq)
    seen, est = [], []
    for q in qs:
        q.register_forward_hook(lambda q, args, out: seen.append((q, args[0].detach().float().cpu(), out.detach())))
    for m in net.modules():
        if hasattr(m, "range_estimator") and m.range_estimator is not None:
            m.range_estimator.register_forward_pre_hook(lambda m, a: est.append(m))
    torch.manual_seed(5)
    xs = [torch.randn(2, 3, 8, 256, device="cuda") * (i + 1) for i in range(2)]
    with torch.no_grad():
        net(xs[0])                                  # "estimating": the quantizers are called directly
        for m in layers:
            m.fix_ranges()
        out = net(xs[1])
    assert out.shape == (2, 8, 6, 134) and torch.isfinite(out).all()
    assert est == [], "no estimator runs for a range_free quantizer"
    assert len(seen) == 8
    from fp8q import ops
    for q, x, y in seen:
        rows = x.reshape(x.shape[0], -1) if (q.flatten_rows and x.dim() > 2) else x
        same(y, ob.oracle(rows.contiguous(), fmt, q.tile)[2].view(x.shape), "a quantizer's output against the oracle")
        same(y, ops.ocp_block_quantize(rows.cuda(), fmt, q.tile).view(x.shape), "the forward equals the op")
    for layer in (net.fc, net.conv):
        q = layer.weight_quantizer.quantizer
        with torch.no_grad():
            w = layer.weight_quantizer(layer.weight)
        back = q.decode(*q.encode(layer.weight.detach())).view(w.shape)
        assert torch.equal(back.view(torch.int32), w.view(torch.int32))
    with pytest.raises(NotImplementedError):
        net(xs[1].requires_grad_(True))


@pytest.mark.parametrize("tile", ob.TILES, ids=_ids)
def test_quantizer_keeps_a_half_dtype_when_asked(tile):
    from quantization.manager import QuantizationManager
    from quantization.ocp import OCPBlockFP8Quantizer
    torch.manual_seed(1)
    x = (torch.randn(6, 2, 132, device="cuda") * 3).bfloat16()
    for keep in (False, True):
        mgr = QuantizationManager(qmethod=OCPBlockFP8Quantizer, qparams=dict(tile=tile, keep_dtype=keep, flatten_rows=True))
        q = mgr.quantizer
        y = mgr(x)                                  # through the manager: the half tensor is not widened on the way
        assert y.dtype == (torch.bfloat16 if keep else torch.float32) and y.shape == x.shape
        ref = ob.oracle(x.float().cpu().view(6, 264), torch.float8_e4m3fn, tile)[2].view(6, 2, 132)
        same(y, ref.to(y.dtype), f"keep_dtype={keep}")
        d = q.decode(*q.encode(x), out_dtype=y.dtype).view(x.shape)
        assert torch.equal(d.view(INT[y.dtype]), y.view(INT[y.dtype]))
