"""The hardware FP8 lane (csrc/fp8q_ocp.hip) against torch's CPU cast, on integers: code bytes, and the bit patterns of
float32 / float16 / bfloat16 values.  No element is left out of any comparison.

The oracle (include/fp8q.h): scale = torch.max(maxval, eps) / fmax; codes = torch.clamp(x / scale, -fmax, fmax).to(fmt);
values = codes.float() * scale.

NaN.  The contract stores every NaN as 0x7F; torch's cast keeps the sign of a NaN (0x7F for float('nan'), 0xFF for its
negative), and which sign a NaN has on the CPU is an accident of the kernels it went through: torch's narrowing of
float('nan') to bfloat16 gives 0xFFFF, and x / NaN came out negative for whole rows of the [4099, 4099] case and positive
in the small ones.  So `_oracle` stores 0x7F wherever the clamped quotient is NaN, and the cast decides everything else.
Where VALUES are compared, a NaN must meet a NaN at the same place, but its
payload is compared in one test only (test_decode_every_code, float32): the payload torch's CPU kernels leave behind after
a multiplication of two NaNs or a narrowing to a half type depends on the operand order and the SIMD path they took
(bfloat16 comes out as 0xFFFF), which is no property of this library.  `_same` maps every NaN to one pattern first.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

FMTS = (torch.float8_e4m3fn, torch.float8_e5m2)
FMAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}
SUB = {torch.float8_e4m3fn: 2.0 ** -9, torch.float8_e5m2: 2.0 ** -16}      # smallest subnormal
EPS = 1e-8
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
SHAPES = [(1, 1), (5, 3), (57, 147), (3, 4100), (2, 3, 7, 7), (8200,)]
CASES = [(s, pc) for s in SHAPES for pc in (False, True) if not (pc and len(s) == 1)]      # [8200] is the per-tensor shape
_id = {torch.float8_e4m3fn: "e4m3fn", torch.float8_e5m2: "e5m2", torch.float32: "f32", torch.float16: "f16",
       torch.bfloat16: "bf16", True: "pc", False: "pt"}


def _ids(v):
    return _id.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else None)


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype in FMAX:
        return t.view(torch.uint8)
    if t.is_floating_point():
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    return t.view(INT[t.dtype])


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, what
    bad = (g != w).flatten().nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {g.numel()} differ, first at {bad[:5].tolist()}: " \
                             f"{g.flatten()[bad[:5]].tolist()} != {w.flatten()[bad[:5]].tolist()}"


def _oracle(x, maxval, fmt, per_channel, eps=EPS):
    """(codes, scale, values) of the contract on the CPU; x float32 (a half input: x.float())"""
    fmax = FMAX[fmt]
    scale = torch.max(maxval.float(), torch.tensor(eps, dtype=torch.float32)) / fmax
    s = scale.view([-1] + [1] * (x.dim() - 1)) if per_channel else scale
    q = torch.clamp(x / s, -fmax, fmax)
    codes = torch.where(torch.isnan(q), torch.tensor(0x7F, dtype=torch.uint8), q.to(fmt).view(torch.uint8)).view(fmt)
    return codes, scale, codes.float() * s


def _case(shape, per_channel, fmt, seed=0):
    """x and maxval on the CPU: seeded normals times per-row magnitudes from 1e-6 to 1e4, ranges below the rows' maxima (so
    elements clip), the special values planted at the front of every row, and -- with three rows or more -- a last row of zeros
    with range 0 (the default eps) and a row before it whose range is NaN"""
    g = torch.Generator().manual_seed(seed)
    C = shape[0] if per_channel else 1
    x = torch.randn(shape, generator=g).reshape(C, -1)
    inner = x.shape[1]
    x = x * (torch.logspace(-6, 4, C).view(C, 1) if C > 1 else 1.0)
    maxval = (x.abs().amax(1) * 0.75).float()
    scale = torch.max(maxval, torch.tensor(EPS)) / FMAX[fmt]
    inf, nan, sub = float("inf"), float("nan"), SUB[fmt]
    for r in range(C):
        mv, s = maxval[r].item(), scale[r].item()
        up = torch.nextafter(maxval[r], torch.tensor(inf)).item()
        plant = [0.0, -0.0, inf, -inf, nan, mv, -mv, up, -up, 2 * mv, 0.4999 * sub * s, -0.4999 * sub * s, 0.5 * sub * s,
                 -0.5001 * sub * s, 1e-45, -1e-45, 1.5 * sub * s, -2.5 * sub * s]
        k = min(inner, len(plant))
        x[r, :k] = torch.tensor(plant[:k])
    if C >= 3:
        x[C - 1] = 0.0
        maxval[C - 1] = 0.0
        maxval[C - 2] = nan
    return x.reshape(shape).contiguous(), maxval


def _check_lane(x, maxval, fmt, per_channel, what, eps=EPS):
    """every entry point on one tensor (x on the CPU, float32 or half) against the oracle of x.float()"""
    from fp8q import ops
    ref_c, ref_s, ref_y = _oracle(x.float(), maxval, fmt, per_channel, eps)
    xd, md = x.cuda(), maxval.cuda()
    codes, scale = ops.ocp_encode(xd, md, fmt, eps=eps)
    assert codes.dtype == fmt and codes.shape == x.shape and scale.dtype == torch.float32
    _same(codes, ref_c, f"{what}: codes")
    _same(scale, ref_s, f"{what}: scale_out")
    _same(ops.ocp_scale(md, fmt, eps), ref_s, f"{what}: ocp_scale")
    outs = [torch.float32] if x.dtype == torch.float32 else [torch.float32, x.dtype]
    for dt in outs:
        y = ops.ocp_quantize(xd, md, fmt, eps=eps, out_dtype=dt)
        assert y.dtype == dt and y.shape == x.shape
        _same(y, ref_y.to(dt), f"{what}: quantize -> {dt}")
        d = ops.ocp_decode(codes, scale, out_dtype=dt)
        # (bit for bit, NaN payloads included: both are this library's)
        assert torch.equal(y.view(INT[dt]), d.view(INT[dt])), f"{what}: quantize != decode(encode) -> {dt}"
    return codes, scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("shape,per_channel", CASES, ids=_ids)
def test_codes_and_values_against_the_cpu_cast(shape, per_channel, fmt, dtype):
    x, maxval = _case(shape, per_channel, fmt)
    _check_lane(x.to(dtype), maxval, fmt, per_channel, f"{shape} {_id[fmt]} {_id[per_channel]} {_id[dtype]}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_unaligned_views_take_the_elementwise_route(fmt, dtype):
    """x.flatten()[1:] of the [57, 147] case: a pointer 4 (2) bytes off the 16-byte grid, codes written to a view 1 byte off"""
    from fp8q import ops
    x, _ = _case((57, 147), False, fmt)
    x = x.to(dtype)
    maxval = torch.tensor([3.0])
    xd = x.cuda().flatten()[1:]
    assert xd.data_ptr() % 16 != 0
    ref_c, ref_s, ref_y = _oracle(x.flatten()[1:].float(), maxval, fmt, False)
    buf = torch.zeros(xd.numel() + 1, dtype=torch.uint8, device="cuda")
    codes, scale = ops.ocp_encode(xd, maxval.cuda(), fmt, eps=EPS, out=buf[1:])
    _same(codes, ref_c, "codes")
    assert buf[0].item() == 0
    ybuf = torch.zeros(xd.numel() + 1, dtype=dtype, device="cuda")
    y = ops.ocp_quantize(xd, maxval.cuda(), fmt, eps=EPS, out=ybuf[1:])
    _same(y, ref_y.to(dtype), "quantize")
    dbuf = torch.zeros(xd.numel() + 1, dtype=dtype, device="cuda")
    d = ops.ocp_decode(codes, scale, out=dbuf[1:])
    assert torch.equal(y.view(INT[dtype]), d.view(INT[dtype]))
    assert ybuf[0].item() == 0 and dbuf[0].item() == 0


def _finite_grid(fmt):
    """the sorted finite values of a format (+-0 once) and the codes of the non-negative ones"""
    v = torch.arange(256, dtype=torch.uint8).view(fmt).float()
    v = v[torch.isfinite(v)]
    return torch.unique(v)          # sorted; -0 == +0 collapse


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_every_midpoint_of_the_grid(fmt):
    """x = midpoint of two neighbouring finite values times scale, and its two float32 neighbours, for every pair: row 0 under a
    power-of-two scale (exact ties: round to even), row 1 with maxval = 3.0 (x / scale lands on or beside the tie: the
    reciprocal route has to redo the division).  Per channel, and each row per tensor."""
    grid = _finite_grid(fmt)
    assert grid.numel() == (253 if fmt == torch.float8_e4m3fn else 247)    # 254 / 248 finite codes, +-0 once
    mid = (grid[:-1] + grid[1:]) / 2
    assert torch.equal(mid.double(), (grid[:-1].double() + grid[1:].double()) / 2)      # exact in float32
    maxval = torch.tensor([FMAX[fmt] * 2.0 ** -5, 3.0])
    scale = maxval / FMAX[fmt]
    rows = []
    for s in scale:
        m = mid * s
        rows.append(torch.cat([m, torch.nextafter(m, torch.tensor(float("inf"))),
                               torch.nextafter(m, torch.tensor(-float("inf"))), grid * s]))
    x = torch.stack(rows).contiguous()
    _check_lane(x, maxval, fmt, True, "midpoints per channel")
    for r in range(2):
        _check_lane(x[r].contiguous(), maxval[r:r + 1], fmt, False, f"midpoints row {r} per tensor")
        _check_lane(x[r].contiguous().bfloat16(), maxval[r:r + 1], fmt, False, f"midpoints row {r} bfloat16")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_midpoints_under_a_subnormal_scale_and_a_huge_range(fmt, dtype):
    """the grid, its midpoints and their float32 neighbours times the scale, clamped to the range, under maxval = 1e-37 (the
    scale is subnormal and 1 / scale overflows: ocp_scale_pair stores a NaN reciprocal and every element is divided) and
    3e38 (a reciprocal near the bottom of the normal range), beside an ordinary row per channel, and each alone per tensor.
    eps = 1e-40, below both, or the default 1e-8 would be the range."""
    eps = 1e-40
    grid = _finite_grid(fmt)
    mid = (grid[:-1] + grid[1:]) / 2
    inf = torch.tensor(float("inf"))
    v = torch.cat([mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf), grid])
    maxval = torch.tensor([1e-37, 3.0, 3e38])
    scale = maxval / FMAX[fmt]
    assert 0 < scale[0].item() < 2.0 ** -126 and torch.isinf(1.0 / scale[0]) and torch.isfinite(1.0 / scale[2])
    x = torch.stack([torch.clamp(v * s, -m, m) for s, m in zip(scale, maxval)]).contiguous().to(dtype)
    assert (x[0] != 0).sum().item() > 300 and torch.isfinite(x).all()      # (bfloat16 under E5M2 keeps 354 of 985 above 0)
    codes, got = _check_lane(x, maxval, fmt, True, "per channel", eps=eps)
    assert torch.equal(got.cpu().view(torch.int32), scale.view(torch.int32))
    for r in (0, 2):
        _check_lane(x[r].contiguous(), maxval[r:r + 1], fmt, False, f"row {r} per tensor", eps=eps)


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_edge_ranges_per_tensor(fmt):
    """all zeros under range 0 (the default eps keeps the scale positive), and a NaN range (every code 0x7F)"""
    x = torch.zeros(300)
    x[1] = -0.0
    _check_lane(x, torch.tensor([0.0]), fmt, False, "zeros")
    x, _ = _case((5, 3), False, fmt)
    codes, _ = _check_lane(x, torch.tensor([float("nan")]), fmt, False, "NaN range")
    assert (codes.view(torch.uint8) == 0x7F).all()


def test_nontemporal_variants_at_4099x4099():
    """67.2 MB of float32: the >= 64 MiB kernels, rows of 4099 elements (no multiple of anything), a partial last chunk"""
    from fp8q import ops
    fmt = torch.float8_e4m3fn
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4099, 4099, generator=g)
    x[5, :3] = torch.tensor([float("nan"), float("inf"), -0.0])
    maxval = x.abs().amax(1) * 0.5
    maxval[7] = float("nan")
    ref_c, ref_s, ref_y = _oracle(x, maxval, fmt, True)
    xd, md = x.cuda(), maxval.cuda()
    codes, scale = ops.ocp_encode(xd, md, fmt, eps=EPS)
    _same(scale, ref_s, "scale_out")
    assert torch.equal(codes.view(torch.uint8).cpu(), ref_c.view(torch.uint8)), "codes"
    y = ops.ocp_quantize(xd, md, fmt, eps=EPS)
    d = ops.ocp_decode(codes, scale)
    assert torch.equal(y.view(torch.int32), d.view(torch.int32))
    _same(y, ref_y, "quantize")


SCALES = [1.0, 2.0 ** -7, 3.0 / 448, 0.75, 1e-6, 1234.5]


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_decode_every_code(fmt):
    """all 256 bytes under several scales, per channel and per tensor, into float32 (exact bits, NaN codes included: they
    decode to the NaN torch's widening gives them) and both half types"""
    from fp8q import ops
    c = torch.arange(256, dtype=torch.uint8).repeat(len(SCALES), 1)
    s = torch.tensor(SCALES)
    ref = c.view(fmt).float() * s.view(-1, 1)
    cd, sd = c.cuda(), s.cuda()
    got = ops.ocp_decode(cd.view(fmt), sd)
    assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32)), "float32, exact bits"
    assert torch.equal(ops.ocp_decode(cd, sd, fmt=fmt).view(torch.int32), got.view(torch.int32)), "uint8 codes with fmt="
    for dt in (torch.float16, torch.bfloat16):
        _same(ops.ocp_decode(cd.view(fmt), sd, out_dtype=dt), ref.to(dt), f"{dt}")
    for i, sc in enumerate(SCALES):
        got1 = ops.ocp_decode(cd[i].contiguous().view(fmt), sd[i:i + 1])
        assert torch.equal(got1.cpu().view(torch.int32), ref[i].view(torch.int32)), f"per tensor, scale {sc}"
    # torch's own conversion on the GPU, times scale
    _same(got, cd.view(fmt).float() * sd.view(-1, 1), "against torch's GPU conversion")


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_encode_of_decode_is_the_identity_on_finite_codes(fmt):
    """encode(decode(c)) == c for every code that is neither NaN nor (E5M2) an infinity: the contract saturates infinities to
    +-fmax, so 0x7C / 0xFC come back as 0x7B / 0xFB, which is asserted too"""
    from fp8q import ops
    c = torch.arange(256, dtype=torch.uint8)
    v = c.view(fmt).float()
    for maxval in (FMAX[fmt] * 0.25, 3.0, 1e-3):
        md = torch.tensor([maxval], device="cuda")
        scale = ops.ocp_scale(md, fmt, EPS)
        y = ops.ocp_decode(c.cuda().view(fmt), scale)
        back = ops.ocp_encode(y, md, fmt, eps=EPS)[0].view(torch.uint8).cpu()
        fin = torch.isfinite(v)
        assert torch.equal(back[fin], c[fin]), f"maxval {maxval}"
        assert (back[torch.isnan(v)] == 0x7F).all()
        if fmt == torch.float8_e5m2:
            assert back[0x7C].item() == 0x7B and back[0xFC].item() == 0xFB


# ---- quantizer, manager, model export --------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3)
        self.fc = torch.nn.Linear(8 * 6 * 6, 10)

    def forward(self, x):
        return self.fc(torch.relu(self.conv(x)).flatten(1))


def _net(fmt, a_est="allminmax"):
    from quantization.layers import QuantizedModule, quantize_model
    from quantization.estimators import RangeEstimators
    from quantization.ocp import OCPFP8Quantizer
    torch.manual_seed(0)
    net = quantize_model(_Net(), method=OCPFP8Quantizer, act_method=OCPFP8Quantizer, n_bits=8, n_bits_act=8,
                         per_channel_weights=True, weight_range_method=RangeEstimators.current_minmax.cls,
                         act_range_method=RangeEstimators[a_est].cls, fp8_kwargs=dict(fmt=fmt)).cuda().eval()
    layers = [m for m in net.modules() if isinstance(m, QuantizedModule)]
    assert tuple(net.conv.weight.shape) == (8, 3, 3, 3) and len(layers) == 2
    for m in layers:
        m.quantized()
        m.estimate_ranges()
    return net, layers


@pytest.mark.parametrize("a_est", ["allminmax", "running_minmax"])
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_model_calibrates_validates_and_exports(fmt, a_est):
    from quantization.model import decode_ocp_weights, export_ocp_weights
    from quantization.ocp import OCPFP8Quantizer
    net, layers = _net(fmt, a_est)
    seen = []

    def hook(q, args, out):
        seen.append((q, args[0].detach().float().cpu(), q.range_maxval.detach().cpu().clone(), out.detach().cpu()))

    qs = [m for m in net.modules() if isinstance(m, OCPFP8Quantizer)]
    assert len(qs) == 4 and all(q.fmt == fmt for q in qs)
    for q in qs:
        q.register_forward_hook(hook)
    torch.manual_seed(5)
    xs = [torch.randn(4, 3, 8, 8, device="cuda") * (i + 1) for i in range(3)]
    with torch.no_grad():
        for x in xs[:2]:
            net(x)                                  # calibration: ranges follow the data
        for m in layers:
            m.fix_ranges()
        out = net(xs[2])                            # validation with fixed ranges
    assert out.shape == (4, 10) and torch.isfinite(out).all()
    assert len(seen) == 12
    for q, x, mv, y in seen:
        assert mv.numel() == (8 if q is net.conv.weight_quantizer.quantizer else 10 if q is net.fc.weight_quantizer.quantizer else 1)
        _same(y, _oracle(x, mv, fmt, q.per_channel)[2], "a quantizer's output against the oracle of its input")
    # export -> decode gives back what the layers compute with
    exp = export_ocp_weights(net)
    assert sorted(exp) == ["conv", "fc"]
    for dt in (None, torch.bfloat16):
        dec = decode_ocp_weights(exp, "cuda", dtype=dt)
        for name, layer in (("conv", net.conv), ("fc", net.fc)):
            e = exp[name]
            assert e["codes"].dtype == fmt and e["fmt"] == fmt and not e["codes"].is_cuda and e["scale"].dtype == torch.float32
            with torch.no_grad():
                wq = layer.weight_quantizer(layer.weight)
            want = wq if dt is None else wq.to(dt)
            assert dec[name].dtype == want.dtype
            assert torch.equal(dec[name].view(INT[want.dtype]), want.view(INT[want.dtype])), (name, dt)
            q = layer.weight_quantizer.quantizer
            assert torch.equal(q.decode(q.encode(layer.weight.detach())).view(torch.int32), wq.view(torch.int32))
    # forward-only: a gradient through a quantizer raises
    with pytest.raises(NotImplementedError):
        net(xs[2].requires_grad_(True))


def test_quantizer_keeps_a_half_dtype_when_asked():
    from quantization.ocp import OCPFP8Quantizer
    x = torch.randn(6, 40, device="cuda").bfloat16()
    for keep in (False, True):
        q = OCPFP8Quantizer(per_channel=True, keep_dtype=keep)
        q.set_quant_range(x.float().amin(1), x.float().amax(1))
        y = q(x)
        assert y.dtype == (torch.bfloat16 if keep else torch.float32)
        ref = _oracle(x.float().cpu(), q.range_maxval.cpu(), torch.float8_e4m3fn, True)[2]
        _same(y, ref.to(y.dtype), f"keep_dtype={keep}")
        assert torch.equal(q.decode(q.encode(x), out_dtype=y.dtype).view(INT[y.dtype]), y.view(INT[y.dtype]))
