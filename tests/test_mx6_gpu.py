"""The 6-bit microscaling formats (E2M3 / E3M2) of csrc/fp8q_mx.hip against the oracle of tests/mx6_oracle.py -- the contract
of include/fp8q.h in exact torch CPU ops.  Every comparison is on integers: the packed code bytes, the scale bytes, and the bit
patterns of float32 / float16 / bfloat16 values with every NaN mapped to one pattern; no element is left out.

Shapes: rows of whole blocks on the 16-byte grid take the vector route (K % 32 == 0), everything else the general one -- ragged
rows whose last block holds a multiple of 4 elements, views off the grid.  K % 4 != 0 is an argument error."""
import functools

import pytest
import torch

import mx6_oracle as mx6
from mx6_oracle import E3M2

pytestmark = pytest.mark.gpu

E8M0 = torch.float8_e8m0fnu
FMTS = mx6.FMTS
ROUNDINGS = ("floor", "ceil")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
SHAPES = [(1, 32), (3, 64), (5, 96),                  # whole blocks
          (1, 4), (2, 28), (7, 36), (4, 148),         # ragged or tiny
          (3, 4128),                                  # rows that cross the 4096-element chunks of the vector route
          (2, 3, 8, 64)]                              # n-D
BAD_SHAPES = [(2, 31), (7, 33)]
_id = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}


def _ids(v):
    return _id.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else None)


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == E8M0:
        return t.view(torch.uint8)
    if t.is_floating_point():
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    return t.view(INT[t.dtype])


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {tuple(g.shape)} {g.dtype} against {tuple(w.shape)} {w.dtype}"
    bad = (g != w).flatten().nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {g.numel()} differ, first at {bad[:5].tolist()}: " \
                             f"{g.flatten()[bad[:5]].tolist()} != {w.flatten()[bad[:5]].tolist()}"


@functools.lru_cache(maxsize=None)
def _case(shape, seed=0):
    """float32 on the CPU: seeded normals times per-row magnitudes from 1e-44 to 1e38, with +-0, +-inf, NaN and +-1e-45
    planted, an all-zero last row (three rows or more) and an all-zero second block in row 0 (K >= 64)"""
    g = torch.Generator().manual_seed(seed)
    K = shape[-1]
    x = torch.randn(shape, generator=g, dtype=torch.float64).reshape(-1, K)
    R = x.shape[0]
    if R > 1:
        x = x * torch.logspace(-44, 38, R, dtype=torch.float64).view(R, 1)
    x = x.float()
    flat = x.view(-1)
    n = flat.numel()
    inf, nan = float("inf"), float("nan")
    for i, v in enumerate([0.0, -0.0, inf, -inf, nan, 1e-45, -1e-45]):
        flat[(41 * i + 3) % n] = v
    if R >= 3:
        x[R - 1] = 0.0
    if K >= 64:
        x[0, 32:64] = 0.0
        x[0, 33] = -0.0
    return x.reshape(shape).contiguous()


@functools.lru_cache(maxsize=None)
def _case_oracle(shape, fmt, rounding, dtype):
    x = _case(shape).to(dtype)
    return (x,) + mx6.oracle(x.float(), fmt, rounding)


def _check_lane(x, ref, fmt, rounding, what):
    """every entry point on one tensor (x on the CPU, float32 or half) against the oracle's (codes, scales, values)"""
    from fp8q import ops
    ref_c, ref_s, ref_y = ref
    xd = x.cuda()
    codes, scales = ops.mx_encode(xd, fmt, rounding)
    assert codes.dtype == torch.uint8 and scales.dtype == E8M0
    assert tuple(codes.shape) == tuple(x.shape[:-1]) + (3 * x.shape[-1] // 4,) == tuple(ref_c.shape)
    assert tuple(scales.shape) == tuple(ref_s.shape)
    _same(scales, ref_s, f"{what}: scales")
    _same(codes, ref_c, f"{what}: codes")
    for dt in ([torch.float32] if x.dtype == torch.float32 else [torch.float32, x.dtype]):
        y = ops.mx_quantize(xd, fmt, rounding, out_dtype=dt)
        assert y.dtype == dt and y.shape == x.shape
        _same(y, ref_y.to(dt), f"{what}: quantize -> {dt}")
        d = ops.mx_decode(codes, scales, fmt=fmt, out_dtype=dt)
        assert d.shape == x.shape and d.dtype == dt
        _same(d, ref_y.to(dt), f"{what}: decode -> {dt}")
        # (bit for bit, NaN payloads included: both are this library's)
        assert torch.equal(y.view(INT[dt]), d.view(INT[dt])), f"{what}: quantize != decode(encode) -> {dt}"
    if rounding == "floor":
        # the operands are a fixed point of the floor rule: encoding what they decode to gives them back
        c2, s2 = ops.mx_encode(ops.mx_decode(codes, scales, fmt=fmt), fmt, "floor")
        _same(s2, ref_s, f"{what}: scales of encode(decode)")
        _same(c2, ref_c, f"{what}: codes of encode(decode)")
    return codes, scales


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_operands_and_values_against_the_oracle(shape, fmt, rounding, dtype):
    x, *ref = _case_oracle(shape, fmt, rounding, dtype)
    _check_lane(x, ref, fmt, rounding, f"{shape} {fmt} {rounding} {_id[dtype]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", BAD_SHAPES, ids=_ids)
def test_a_row_length_that_is_no_multiple_of_4_raises(shape, fmt, dtype):
    """four elements share three bytes: FP8Q_EINVAL at the C ABI, a geometry error here, never a launch"""
    from fp8q import ops
    x = _case(shape).to(dtype).cuda()
    for rounding in ROUNDINGS:
        with pytest.raises(ops.Fp8qError, match="multiple of 4"):
            ops.mx_encode(x, fmt, rounding)
        with pytest.raises(ops.Fp8qError, match="multiple of 4"):
            ops.mx_quantize(x, fmt, rounding)
    n = shape[-1] + (shape[-1] % 3 == 0)                            # a code length that is no multiple of 3
    with pytest.raises(ops.Fp8qError, match="multiple of 3"):
        ops.mx_decode(torch.zeros(shape[:-1] + (n,), dtype=torch.uint8, device="cuda"),
                      torch.zeros(shape[:-1] + (2,), dtype=torch.uint8, device="cuda"), fmt=fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_every_midpoint_of_the_grid(fmt):
    """for each of the 31 gaps between neighbouring magnitudes: the midpoint, its float32 neighbours below and above, and the
    three negated, in blocks that an anchor 2^emax * X pins to the scale X (either rounding: the anchor's mantissa is 0), for
    X = 1 and X = 2^-20; as float32, and as bfloat16, which holds every midpoint"""
    grid = mx6.element_value(torch.arange(32), fmt)
    assert grid.numel() == 32 and bool((grid[1:] > grid[:-1]).all()) and grid[-1].item() == mx6.FMAX[fmt]
    mid = (grid[:-1] + grid[1:]) / 2
    assert torch.equal(mid.double(), (grid[:-1].double() + grid[1:].double()) / 2)      # exact in float32
    inf = torch.tensor(float("inf"))
    for code in (127, 107):
        X = mx6.pow2(torch.tensor(code - 127))
        m = mid * X
        assert torch.equal(m.double(), mid.double() * X.double())
        pos = torch.cat([m, torch.nextafter(m, -inf), torch.nextafter(m, inf)])
        vals = torch.cat([pos, -pos])
        assert vals.numel() == 31 * 6
        x = torch.cat([(2.0 ** mx6.EMAX[fmt] * X).expand(6, 1), vals.view(6, 31)], 1).contiguous()
        for rounding in ROUNDINGS:
            ref = mx6.oracle(x, fmt, rounding)
            assert (ref[1] == code).all()
            # the oracle against the rule said once more: a midpoint goes to the even code, its neighbours to theirs
            c = mx6.unpack(ref[0])
            lo = torch.arange(31)
            assert torch.equal(c[0, 1:], lo + (lo % 2)) and torch.equal(c[1, 1:], lo) and torch.equal(c[2, 1:], lo + 1)
            assert torch.equal(c[3:, 1:], c[:3, 1:] | 32)
            _check_lane(x, ref, fmt, rounding, f"midpoints {fmt} code {code} {rounding}")
            xb = x.bfloat16()
            assert torch.equal(xb.float()[0, 1:], m)
            _check_lane(xb, mx6.oracle(xb.float(), fmt, rounding), fmt, rounding, f"midpoints bf16 {fmt} code {code} {rounding}")


SCALE_CODES = (0, 1, 126, 127, 128, 254, 255)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_every_code(fmt):
    """all 64 codes under the scale bytes 0, 1, 126, 127, 128, 254 and 255, into float32 and both half types: as rows of 64
    elements in 48 bytes (the vector route) and cut to rows of 40 in 30 bytes (block by block, a short last block)"""
    from fp8q import ops
    n = len(SCALE_CODES)
    c = torch.arange(64).repeat(n, 1)
    b = mx6.pack(c)
    s = torch.tensor(SCALE_CODES, dtype=torch.uint8).view(-1, 1).repeat(1, 2)
    ref = mx6.element_value(c, fmt) * mx6.scale_value(torch.tensor(SCALE_CODES)).view(-1, 1)
    assert torch.equal(_bits(mx6.decode(b, s, fmt)), _bits(ref))
    assert torch.isnan(ref[-1]).all() and not torch.isnan(ref[:-1]).any()
    bd, sd = b.cuda(), s.cuda()
    got = ops.mx_decode(bd, sd, fmt=fmt)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 64)
    _same(got, ref, "float32")
    assert torch.equal(ops.mx_decode(bd, sd.view(E8M0), fmt=fmt).view(torch.int32), got.view(torch.int32)), "e8m0 scales"
    for dt in (torch.float16, torch.bfloat16):
        _same(ops.mx_decode(bd, sd, fmt=fmt, out_dtype=dt), ref.to(dt), f"{dt}")
    b40, s40 = b[:, :30].contiguous().cuda(), s.cuda()
    for dt in DTYPES:
        _same(ops.mx_decode(b40, s40, fmt=fmt, out_dtype=dt), ref[:, :40].contiguous().to(dt), f"rows of 40 -> {dt}")


def _ladder(fmt):
    """[3 * 256, 32]: blocks whose largest element has the exponent field 0 .. 255 and the mantissa one below man_fmax, man_fmax
    and one above -- where `ceil` bumps; E = 255 makes them NaNs -- at a position and with a sign that change from block to
    block, over elements a quarter of it (those of the NaN blocks are 1)"""
    e = torch.arange(256).repeat_interleave(3)
    man = torch.tensor([mx6.MAN_FMAX[fmt] - 1, mx6.MAN_FMAX[fmt], mx6.MAN_FMAX[fmt] + 1]).repeat(256)
    top = ((e << 23) | man).to(torch.int32).view(torch.float32)
    x = torch.where(e == 255, torch.ones_like(top), top * 0.25).view(-1, 1).repeat(1, 32)
    i = torch.arange(top.numel())
    x[i, i % 32] = top * torch.where(i % 2 == 1, -1.0, 1.0)
    return x.contiguous(), e, man


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("fmt", FMTS)
def test_scale_ladder(fmt, rounding):
    x, e, man = _ladder(fmt)
    ref = mx6.oracle(x, fmt, rounding)
    want = torch.clamp(e - mx6.EMAX[fmt] + ((man > mx6.MAN_FMAX[fmt]).long() if rounding == "ceil" else 0), min=0)
    want = torch.where(e == 255, torch.tensor(255), want)
    assert torch.equal(ref[1].flatten().long(), want)            # the oracle against the rule written out once more
    _check_lane(x, ref, fmt, rounding, f"ladder {fmt} {rounding}")
    x4 = x.view(-1, 128)
    _check_lane(x4, mx6.oracle(x4, fmt, rounding), fmt, rounding, f"ladder as rows of four blocks {fmt} {rounding}")
    x36 = x.reshape(-1, 64)[:, :36].contiguous()                 # a whole block and four elements of the next
    _check_lane(x36, mx6.oracle(x36, fmt, rounding), fmt, rounding, f"ladder as rows of 36 {fmt} {rounding}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("fmt", FMTS)
def test_unaligned_and_ragged_views_take_the_general_route(fmt, dtype):
    """x.flatten()[1:] as [5, 32]: a pointer 4 (2) bytes off the 16-byte grid; the codes written to, and read from, a view one
    byte into its buffer, where no three-byte group lies in one aligned dword; values written one element off; rows of 36; the
    bytes on either side of every output untouched"""
    from fp8q import ops
    k = 5
    base = _case((1, 32 * k + 1)).to(dtype)
    x = base.flatten()[1:].reshape(k, 32)
    ref_c, ref_s, ref_y = mx6.oracle(x.float(), fmt, "floor")
    xd = base.cuda().flatten()[1:].view(k, 32)
    assert xd.data_ptr() % 16 != 0
    cbuf = torch.full((ref_c.numel() + 2,), 0xA5, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((ref_s.numel() + 2,), 0xA5, dtype=torch.uint8, device="cuda")
    codes, scales = ops.mx_encode(xd, fmt, out=cbuf[1:-1], scales_out=sbuf[1:-1])
    assert codes.data_ptr() == cbuf.data_ptr() + 1 and tuple(codes.shape) == (k, 24)
    _same(codes, ref_c, "codes")
    _same(scales, ref_s, "scales")
    ybuf = torch.full((x.numel() + 2,), 7.0, dtype=dtype, device="cuda")
    y = ops.mx_quantize(xd, fmt, out=ybuf[1:-1])
    _same(y.view(k, 32), ref_y.to(dtype), "quantize")
    dbuf = torch.full((x.numel() + 2,), 7.0, dtype=dtype, device="cuda")
    d = ops.mx_decode(codes, scales, fmt=fmt, out=dbuf[1:-1])
    assert torch.equal(y.view(INT[dtype]), d.view(INT[dtype]))
    # an aligned x, the codes alone one byte off
    xa = x.contiguous().cuda()
    assert xa.data_ptr() % 16 == 0
    cbuf2 = torch.full((ref_c.numel() + 2,), 0xA5, dtype=torch.uint8, device="cuda")
    codes2, scales2 = ops.mx_encode(xa, fmt, out=cbuf2[1:-1])
    _same(codes2, ref_c, "codes one byte off")
    _same(scales2, ref_s, "their scales")
    _same(ops.mx_decode(codes2, scales2, fmt=fmt, out_dtype=dtype), ref_y.to(dtype), "decode of codes one byte off")
    for buf, v in ((cbuf, 0xA5), (cbuf2, 0xA5), (sbuf, 0xA5), (ybuf, 7.0), (dbuf, 7.0)):
        assert buf[0].item() == v and buf[-1].item() == v
    # K = 36: every row is a whole block and a block of four
    x36 = _case((7, 36)).to(dtype)
    r36 = mx6.oracle(x36.float(), fmt, "ceil")
    cbuf3 = torch.full((r36[0].numel() + 2,), 0xA5, dtype=torch.uint8, device="cuda")
    c36, s36 = ops.mx_encode(x36.cuda(), fmt, "ceil", out=cbuf3[1:-1])
    _same(c36, r36[0], "codes of rows of 36")
    _same(s36, r36[1], "scales of rows of 36")
    _same(ops.mx_decode(c36, s36, fmt=fmt, out_dtype=dtype), r36[2].to(dtype), "decode of rows of 36")
    assert cbuf3[0].item() == 0xA5 and cbuf3[-1].item() == 0xA5


@functools.lru_cache(maxsize=None)
def _big():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4100, 4128, generator=g) * torch.logspace(-30, 30, 4100).view(-1, 1)
    x[5, :3] = torch.tensor([float("nan"), float("inf"), -0.0])
    x[4099, 4096:] = 0.0
    return x, x.cuda()


@pytest.mark.parametrize("fmt", FMTS)
def test_nontemporal_variants_at_4100x4128(fmt):
    """67.7 MB of float32: the >= 64 MiB kernels of the vector route, rows of 129 blocks, a partial last chunk"""
    from fp8q import ops
    x, xd = _big()
    ref_c, ref_s, ref_y = mx6.oracle(x, fmt, "floor")
    codes, scales = ops.mx_encode(xd, fmt)
    assert tuple(codes.shape) == (4100, 3096)
    assert torch.equal(scales.view(torch.uint8).cpu(), ref_s), "scales"
    assert torch.equal(codes.cpu(), ref_c), "codes"
    y = ops.mx_quantize(xd, fmt)
    d = ops.mx_decode(codes, scales, fmt=fmt)
    assert torch.equal(y.view(torch.int32), d.view(torch.int32))
    _same(y, ref_y, "quantize")


# ---- quantizer, manager, model export --------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(64, 48)
        self.conv = torch.nn.Conv2d(4, 8, 3)

    def forward(self, x):                     # [N, 4, 8, 64] -> [N, 4, 8, 48] -> [N, 8, 6, 46]
        return self.conv(torch.relu(self.fc(x)))


def _net(fmt, rounding):
    from quantization.layers import QuantizedModule, quantize_model
    from quantization.estimators import RangeEstimators
    from quantization.mx import MXQuantizer
    torch.manual_seed(0)
    net = quantize_model(_Net(), method=MXQuantizer, act_method=MXQuantizer, n_bits=6, n_bits_act=6,
                         per_channel_weights=True, weight_range_method=RangeEstimators.current_minmax.cls,
                         act_range_method=RangeEstimators.running_minmax.cls,
                         fp8_kwargs=dict(fmt=fmt, rounding=rounding, flatten_rows=True)).cuda().eval()
    layers = [m for m in net.modules() if isinstance(m, QuantizedModule)]
    assert tuple(net.conv.weight.shape) == (8, 4, 3, 3) and len(layers) == 2
    for m in layers:
        m.quantized()
        m.estimate_ranges()
    return net, layers


def test_model_quantizes_and_exports():
    """a Linear and a convolution under E3M2 with flatten_rows: weight rows of 64 and of 4 * 3 * 3 = 36 elements, activations
    as [N, -1].  Every quantizer's output is the oracle's value of its input, so the forward is that of the same net with its
    weights and activations replaced by oracle values; the exported operands decode to the layers' quantized weights"""
    from quantization.model import decode_mx_weights, export_mx_weights
    from quantization.mx import MXQuantizer
    fmt, rounding = E3M2, "floor"
    net, layers = _net(fmt, rounding)
    seen = []

    def hook(q, args, out):
        seen.append((q, args[0].detach().float().cpu(), out.detach().cpu()))

    qs = [m for m in net.modules() if isinstance(m, MXQuantizer)]
    assert len(qs) == 4 and all(q.fmt == fmt and q.n_bits == 6 and q.rounding == rounding and q.flatten_rows for q in qs)
    for q in qs:
        q.register_forward_hook(hook)
    torch.manual_seed(5)
    xs = [torch.randn(2, 4, 8, 64, device="cuda") * (i + 1) for i in range(2)]
    with torch.no_grad():
        net(xs[0])                                  # "estimating": the quantizers are called directly
        for m in layers:
            m.fix_ranges()                          # nothing to fix, nothing refuses
        out = net(xs[1])
    assert out.shape == (2, 8, 6, 46) and torch.isfinite(out).all()
    assert len(seen) == 8
    for q, x, y in seen:
        rows = x.reshape(x.shape[0], -1) if x.dim() > 2 else x
        want = mx6.oracle(rows.contiguous(), fmt, rounding)[2].view(x.shape)
        _same(y, want, "a quantizer's output against the oracle of its input")
    exp = export_mx_weights(net)
    assert sorted(exp) == ["conv", "fc"]
    assert tuple(exp["conv"]["codes"].shape) == (8, 27) and tuple(exp["conv"]["scales"].shape) == (8, 2)
    assert tuple(exp["fc"]["codes"].shape) == (48, 48) and tuple(exp["fc"]["scales"].shape) == (48, 2)
    for name, layer in (("conv", net.conv), ("fc", net.fc)):
        e = exp[name]
        assert e["codes"].dtype == torch.uint8 and e["fmt"] == "e3m2" and e["scales"].dtype == E8M0 and not e["codes"].is_cuda
        w = layer.weight.detach().float().cpu()
        ref_c, ref_s, _ = mx6.oracle(w.reshape(w.shape[0], -1).contiguous(), fmt, rounding)
        _same(e["codes"], ref_c, f"{name}: exported codes")
        _same(e["scales"], ref_s, f"{name}: exported scales")
    for dt in (None, torch.bfloat16):
        dec = decode_mx_weights(exp, "cuda", dtype=dt)
        for name, layer in (("conv", net.conv), ("fc", net.fc)):
            with torch.no_grad():
                wq = layer.weight_quantizer(layer.weight)
            want = wq if dt is None else wq.to(dt)
            assert dec[name].dtype == want.dtype and dec[name].shape == want.shape
            assert torch.equal(dec[name].view(INT[want.dtype]), want.view(INT[want.dtype])), (name, dt)
            q = layer.weight_quantizer.quantizer
            back = q.decode(*q.encode(layer.weight.detach())).view(wq.shape)
            assert torch.equal(back.view(torch.int32), wq.view(torch.int32))
    # forward-only: a gradient through a quantizer raises
    with pytest.raises(NotImplementedError):
        net(xs[1].requires_grad_(True))


@pytest.mark.parametrize("fmt", FMTS)
def test_quantizer_keeps_a_half_dtype_when_asked(fmt):
    """a bfloat16 tensor through the manager: float32 out, or bfloat16 with keep_dtype (the float32 value rounded once); its
    operands are those of the exactly widened tensor"""
    from quantization.manager import QuantizationManager
    from quantization.mx import MXQuantizer
    torch.manual_seed(1)
    x = (torch.randn(6, 2, 40, device="cuda") * 3).bfloat16()
    for keep in (False, True):
        mgr = QuantizationManager(qmethod=MXQuantizer, qparams=dict(fmt=fmt, keep_dtype=keep, flatten_rows=True))
        q = mgr.quantizer
        y = mgr(x)                                  # through the manager: the half tensor is not widened on the way
        assert y.dtype == (torch.bfloat16 if keep else torch.float32) and y.shape == x.shape
        ref = mx6.oracle(x.float().cpu().view(6, 80), fmt, "floor")[2].view(6, 2, 40)
        _same(y, ref.to(y.dtype), f"keep_dtype={keep}")
        codes, scales = q.encode(x)
        assert codes.dtype == torch.uint8 and tuple(codes.shape) == (6, 60)
        d = q.decode(codes, scales, out_dtype=y.dtype).view(x.shape)
        assert torch.equal(d.view(INT[y.dtype]), y.view(INT[y.dtype]))
