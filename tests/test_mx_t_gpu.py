"""The MX lane with the blocks along dim 0 (csrc/fp8q_mx_t.hip: ops.mx_encode_t / mx_encode_both / mx_quantize_t and
MXQuantizer(block_axis=-2)) against the CPU oracle of the contract applied to the transposed tensor: the transposed operands of
x are defined as the operands of the contiguous x.t().  E4M3FN, E5M2 and E2M1 use an oracle written here in torch integer ops
as include/fp8q.h reads; the 6-bit formats use tests/mx6_oracle.py.  Every comparison is on integers -- code bytes, scale
bytes, the bit patterns of values with every NaN mapped to one pattern -- and no element is left out.

Shapes that straddle a tile edge are derived from the tile fp8q_mxt_route reports, and every case asserts its route first.
Where a format's packing cannot take a shape (E2M1: an odd R, FP6: R % 4; encode_both: the same of K), the encoders must
raise; quantize_t packs nothing, so it is still checked there, against the oracle of x.t() padded with zero columns to a
multiple of 4 (the contract zero-pads the last block anyway, so the values of the real elements are the same).
"""
import functools

import pytest
import torch

import mx6_oracle as mx6

pytestmark = pytest.mark.gpu

E4M3, E5M2, E2M1, E2M3, E3M2 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2, "e2m3", "e3m2"
E8M0 = torch.float8_e8m0fnu
FMTS = (E4M3, E5M2, E2M1, E2M3, E3M2)
FP6 = (E2M3, E3M2)
ROUNDINGS = ("floor", "ceil")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
EMAX = {E4M3: 8, E5M2: 15, E2M1: 2}
FMAX = {E4M3: 448.0, E5M2: 57344.0, E2M1: 6.0}
MAN_FMAX = {E4M3: 0x600000, E5M2: 0x600000, E2M1: 0x400000}
FP4_VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
FP4_MIDS = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
MULT = {E4M3: 1, E5M2: 1, E2M1: 2, E2M3: 4, E3M2: 4}           # elements that share whole bytes
_id = {E4M3: "e4m3fn", E5M2: "e5m2", E2M1: "e2m1", E2M3: "e2m3", E3M2: "e3m2", torch.float32: "f32", torch.float16: "f16",
       torch.bfloat16: "bf16"}


def _ids(v):
    return _id.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else None)


def _tile():
    from fp8q import ops
    r = ops.mx_t_route(64, 128, E4M3, torch.float32)
    assert r["kernel"] == "tile" and r["tile_rows"] % 32 == 0 and r["tile_cols"] % 4 == 0
    return r["tile_rows"], r["tile_cols"]


def _shapes():
    """(R, K, the route a float32 tensor must take)"""
    TR, TC = _tile()
    tile = [(32, 4), (32, TC), (TR, TC), (TR + 32, 2 * TC + 4), (31, 64), (33, 128), (1, 32), (2 * TR + 36, TC + 8), (300, 260)]
    general = [(64, 33), (40, 1), (7, 3)]
    return [(R, K, "tile") for R, K in tile] + [(R, K, "general") for R, K in general]


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype in (E4M3, E5M2, E2M1, E8M0):
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


def _pow2(n):
    return ((n + 127) << 23).to(torch.int32).view(torch.float32)


def _scale_value(code):
    b = torch.where(code == 0, torch.tensor(0x00400000), torch.where(code == 255, torch.tensor(0x7FC00000), code << 23))
    return b.to(torch.int32).view(torch.float32)


def _fp4_codes(q):
    a = q.abs()
    cnt = (a.unsqueeze(-1) > FP4_MIDS).sum(-1)
    tie = (a.unsqueeze(-1) == FP4_MIDS).any(-1) & (cnt % 2 == 1)
    return (cnt + tie.long()) | ((q.view(torch.int32) < 0).long() << 3)


def _fp4_value(c):
    return FP4_VALUES[c & 7] * torch.where((c & 8) != 0, -1.0, 1.0)


def _oracle8(x, fmt, rounding):
    """(codes uint8, scales uint8, values float32) of the contract for E4M3FN / E5M2 / E2M1; x float32 [rows, K] on the CPU,
    blocks along the last dimension (E2M1: K even)"""
    assert x.dtype == torch.float32 and not x.is_cuda and x.dim() == 2
    rows, K = x.shape
    nb = (K + 31) // 32
    xp = torch.zeros(rows, nb * 32)
    xp[:, :K] = x
    xb = xp.view(rows, nb, 32)
    m = (xb.view(torch.int32) & 0x7FFFFFFF).amax(-1).long()           # non-negative int32: signed order == unsigned order
    E, man = m >> 23, m & 0x7FFFFF
    bump = (man > MAN_FMAX[fmt]).long() if rounding == "ceil" else torch.zeros_like(E)
    code = torch.clamp(E - EMAX[fmt] + bump, min=0)
    code = torch.where(E == 255, torch.tensor(255), code)
    nanb = (code == 255).unsqueeze(-1)
    inv = _pow2(torch.where(code == 255, torch.tensor(0), 127 - code)).unsqueeze(-1)
    q = torch.clamp(xb * inv, -FMAX[fmt], FMAX[fmt])
    q = torch.where(nanb, torch.zeros_like(q), q)
    X = _scale_value(code).unsqueeze(-1)
    if fmt == E2M1:
        c = torch.where(nanb, torch.tensor(0), _fp4_codes(q))
        vals = _fp4_value(c) * X
        c = c.view(rows, nb * 32)[:, :K]
        codes = (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)
    else:
        c = torch.where(nanb, torch.tensor(0x7F, dtype=torch.uint8), q.to(fmt).view(torch.uint8))
        vals = c.view(fmt).float() * X
        codes = c.view(rows, nb * 32)[:, :K]
    vals = vals.view(rows, nb * 32)[:, :K].contiguous()
    return codes.contiguous(), code.to(torch.uint8), vals


def _oracle(x, fmt, rounding):
    """(codes or None, scales, values) of the contract on x [rows, K]; codes None where K does not pack into whole bytes -- the
    values then come from x padded with zero columns, which the contract's own zero padding of the last block makes equal"""
    rows, K = x.shape
    fn = (lambda t: mx6.oracle(t, fmt, rounding)) if fmt in FP6 else (lambda t: _oracle8(t, fmt, rounding))
    if K % MULT[fmt] == 0:
        return fn(x)
    xp = torch.zeros(rows, (K + 3) // 4 * 4)
    xp[:, :K] = x
    _, s, v = fn(xp)
    return None, s, v[:, :K].contiguous()


def test_the_oracle_on_values_written_down_by_hand():
    """no library code: the transposed contract on a column whose operands can be written down"""
    x = torch.zeros(40, 2)
    x[:10, 0] = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.0])          # E = 129: code 127, X = 1
    x[32:36, 1] = torch.tensor([480.0, 1.0625, 1.1875, float(2 ** -10)])
    c, s, v = _oracle(x.t().contiguous(), E2M1, "floor")
    assert tuple(c.shape) == (2, 20) and tuple(s.shape) == (2, 2) and s[0].tolist() == [127, 0]
    nib = torch.stack([c[0] & 15, c[0] >> 4], -1).flatten()[:10].tolist()
    assert nib == [6, 0, 2, 2, 4, 4, 6, 6, 8, 8]
    c, s, v = _oracle(x.t().contiguous(), E4M3, "floor")
    assert s[1].tolist() == [0, 127] and c[1, 32:36].tolist() == [0x7E, 0x38, 0x3A, 0x00]
    c, s, v = _oracle(x.t().contiguous(), E4M3, "ceil")
    assert s[1].tolist() == [0, 128] and v[1, 32].item() == 480.0
    # an unpackable length: the values of the padded tensor are the values
    c, s, v = _oracle(x[:39].t().contiguous(), E2M1, "floor")
    assert c is None and tuple(v.shape) == (2, 39) and v[0, :10].tolist() == [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -0.0, -0.0]


@functools.lru_cache(maxsize=None)
def _case_t(shape, seed=0):
    """float32 [K, R] on the CPU, the transpose of the input: seeded normals times per-row magnitudes from 1e-44 to 1e38 -- so
    the ladder runs across x's columns and every block along R holds comparable values -- with +-0, +-inf, NaN and +-1e-45
    planted, an all-zero last row (an all-zero column of x; three columns or more) and an all-zero second block in row 0 (an
    all-zero block of 32 rows in column 0 of x; R >= 64)"""
    g = torch.Generator().manual_seed(seed)
    K, R = shape
    xt = torch.randn(shape, generator=g, dtype=torch.float64)
    if K > 1:
        xt = xt * torch.logspace(-44, 38, K, dtype=torch.float64).view(K, 1)
    xt = xt.float()
    flat = xt.view(-1)
    n = flat.numel()
    inf, nan = float("inf"), float("nan")
    for i, v in enumerate([0.0, -0.0, inf, -inf, nan, 1e-45, -1e-45]):
        flat[(41 * i + 3) % n] = v
    if K >= 3:
        xt[K - 1] = 0.0
    if R >= 64:
        xt[0, 32:64] = 0.0
        xt[0, 33] = -0.0
    return xt.contiguous()


@functools.lru_cache(maxsize=None)
def _case(R, K, dtype):
    """(x [R, K] of dtype, x.t() as contiguous float32) on the CPU"""
    x = _case_t((K, R)).t().contiguous().to(dtype)
    return x, x.float().t().contiguous()


@functools.lru_cache(maxsize=None)
def _ref(R, K, dtype, fmt, rounding, transposed):
    x, xt = _case(R, K, dtype)
    return _oracle(xt if transposed else x.float(), fmt, rounding)


def _route_of(R, K, dtype, aligned=True):
    return "tile" if aligned and K % (4 if dtype == torch.float32 else 8) == 0 else "general"


def _check(xd, R, K, dtype, fmt, rounding, what):
    """every entry on one device tensor x [R, K] against the oracles of x and of x.t()"""
    from fp8q import ops
    ct, st, vt = _ref(R, K, dtype, fmt, rounding, True)
    cdt = torch.uint8 if fmt in FP6 else fmt
    dts = [torch.float32] if dtype == torch.float32 else [torch.float32, dtype]
    can_t, can_both = R % MULT[fmt] == 0, R % MULT[fmt] == 0 and K % MULT[fmt] == 0
    ys = {}
    for dt in dts:
        y = ops.mx_quantize_t(xd, fmt, rounding, out_dtype=dt)
        assert y.dtype == dt and tuple(y.shape) == (R, K) and y.is_contiguous()
        _same(y, vt.t().to(dt), f"{what}: quantize_t -> {dt}")
        ys[dt] = y
    if not can_t:
        # a checked outcome, not a skip: codes that cannot be packed along R are an argument error
        with pytest.raises(ops.Fp8qError):
            ops.mx_encode_t(xd, fmt, rounding)
        with pytest.raises(ops.Fp8qError):
            ops.mx_encode_both(xd, fmt, rounding)
        return
    codes_t, scales_t = ops.mx_encode_t(xd, fmt, rounding)
    assert codes_t.dtype == cdt and scales_t.dtype == E8M0
    assert tuple(codes_t.shape) == tuple(ct.shape) and tuple(scales_t.shape) == tuple(st.shape) == (K, (R + 31) // 32)
    _same(scales_t, st, f"{what}: scales_t")
    _same(codes_t, ct, f"{what}: codes_t")
    # the existing kernels on the transposed copy: byte for byte
    c2, s2 = ops.mx_encode(xd.t().contiguous(), fmt, rounding)
    assert torch.equal(c2.view(torch.uint8), codes_t.view(torch.uint8)) and torch.equal(s2.view(torch.uint8), scales_t.view(torch.uint8))
    for dt in dts:
        d = ops.mx_decode(codes_t, scales_t, fmt=fmt if fmt in FP6 else None, out_dtype=dt).t()
        assert torch.equal(d.contiguous().view(INT[dt]), ys[dt].view(INT[dt])), f"{what}: quantize_t != decode(encode_t).t() -> {dt}"
    if rounding == "floor":
        back = ops.mx_decode(codes_t, scales_t, fmt=fmt if fmt in FP6 else None).t().contiguous()
        c3, s3 = ops.mx_encode_t(back, fmt, "floor")
        _same(s3, st, f"{what}: scales_t of encode_t(decode)")
        _same(c3, ct, f"{what}: codes_t of encode_t(decode)")
    if not can_both:
        with pytest.raises(ops.Fp8qError):
            ops.mx_encode_both(xd, fmt, rounding)
        return
    cr, sr, _ = _ref(R, K, dtype, fmt, rounding, False)
    codes, scales, codes_b, scales_b = ops.mx_encode_both(xd, fmt, rounding)
    assert codes.dtype == cdt and scales.dtype == E8M0 and codes_b.dtype == cdt and scales_b.dtype == E8M0
    _same(scales, sr, f"{what}: encode_both scales")
    _same(codes, cr, f"{what}: encode_both codes")
    _same(scales_b, st, f"{what}: encode_both scales_t")
    _same(codes_b, ct, f"{what}: encode_both codes_t")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("idx", range(12))
def test_operands_and_values_against_the_oracle_of_the_transpose(idx, fmt, rounding, dtype):
    from fp8q import ops
    shapes = _shapes()
    assert len(shapes) == 12
    R, K, route = shapes[idx]
    if dtype == torch.float32:
        assert _route_of(R, K, dtype) == route
    assert ops.mx_t_route(R, K, fmt, dtype)["kernel"] == _route_of(R, K, dtype), "route"
    x, _ = _case(R, K, dtype)
    xd = x.cuda()
    assert xd.data_ptr() % 16 == 0
    _check(xd, R, K, dtype, fmt, rounding, f"[{R}, {K}] {_id[fmt]} {rounding} {_id[dtype]}")


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_a_view_off_the_16_byte_grid_takes_the_general_route(fmt, rounding):
    from fp8q import ops
    R, K = 64, 128
    x, _ = _case(R, K, torch.float32)
    base = torch.zeros(R * K + 8, device="cuda")
    base[1:1 + R * K] = x.flatten().cuda()
    xd = base[1:1 + R * K].view(R, K)
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    assert ops.mx_t_route(R, K, fmt, torch.float32, aligned16=False)["kernel"] == "general"
    assert ops.mx_t_route(R, K, fmt, torch.float32)["kernel"] == "tile"
    _check(xd, R, K, torch.float32, fmt, rounding, f"misaligned {_id[fmt]} {rounding}")


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_a_half_tensor_with_k_36_takes_the_general_route(fmt, dtype):
    from fp8q import ops
    R, K = 40, 36
    assert ops.mx_t_route(R, K, fmt, dtype)["kernel"] == "general" and ops.mx_t_route(R, K, fmt, torch.float32)["kernel"] == "tile"
    x, _ = _case(R, K, dtype)
    _check(x.cuda(), R, K, dtype, fmt, "floor", f"[40, 36] {_id[fmt]} {_id[dtype]}")


def _big(R, K, dtype):
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(R, K, generator=g, device="cuda") * torch.logspace(-30, 30, K, device="cuda").view(1, -1)
    x[:3, 5] = torch.tensor([float("nan"), float("inf"), -0.0], device="cuda")
    x[4096:, K - 1] = 0.0
    return x.to(dtype)


@pytest.mark.parametrize("R,K,dtype,route,nt", [(4128, 4100, torch.float32, "tile", True), (4128, 4100, torch.bfloat16, "general", False),
                                                (4128, 4104, torch.bfloat16, "tile", True)],
                         ids=["4128x4100-f32", "4128x4100-bf16", "4128x4104-bf16"])
def test_nontemporal_variants_against_the_existing_kernels(R, K, dtype, route, nt):
    """67.7 MB of float32-sized elements: the >= 64 MiB kernels, a ragged last tile in both directions (the existing lane's
    4100x4128 rule with the axes swapped).  The comparator is the existing lane on the transposed copy, which its own tests hold
    to the oracle, so no CPU oracle of 17 M elements is needed.  K = 4100 is no multiple of 8: a bfloat16 tensor of that shape
    goes block by block, so the bfloat16 tile kernel's nontemporal variant gets K = 4104."""
    from fp8q import ops
    x = _big(R, K, dtype)
    xt = x.t().contiguous()
    for fmt in (E4M3, E2M1, E2M3):
        r = ops.mx_t_route(R, K, fmt, dtype)
        assert r["kernel"] == route and r["nontemporal"] == nt, r
        want_ct, want_st = ops.mx_encode(xt, fmt)
        ct, st = ops.mx_encode_t(x, fmt)
        assert torch.equal(st.view(torch.uint8), want_st.view(torch.uint8)), f"{_id[fmt]}: scales_t"
        assert torch.equal(ct.view(torch.uint8), want_ct.view(torch.uint8)), f"{_id[fmt]}: codes_t"
        want_c, want_s = ops.mx_encode(x, fmt)
        c, s, ct2, st2 = ops.mx_encode_both(x, fmt)
        assert torch.equal(s.view(torch.uint8), want_s.view(torch.uint8)) and torch.equal(c.view(torch.uint8), want_c.view(torch.uint8))
        assert torch.equal(st2.view(torch.uint8), want_st.view(torch.uint8)) and torch.equal(ct2.view(torch.uint8), want_ct.view(torch.uint8))
        for dt in ([torch.float32] if dtype == torch.float32 else [torch.float32, dtype]):
            want_y = ops.mx_quantize(xt, fmt, out_dtype=dt).t().contiguous()
            y = ops.mx_quantize_t(x, fmt, out_dtype=dt)
            assert torch.equal(y.view(INT[dt]), want_y.view(INT[dt])), f"{_id[fmt]}: quantize_t -> {dt}"
        del want_ct, want_st, ct, st, c, s, ct2, st2, want_c, want_s, want_y, y


def test_out_tensors_are_validated_and_nothing_is_launched():
    from fp8q import ops
    R, K = 64, 128
    x = _case(R, K, torch.float32)[0].cuda()
    nb = 2
    good_c = lambda: torch.full((K, R), 0xA5, dtype=torch.uint8, device="cuda")           # noqa: E731
    good_s = lambda: torch.full((K, nb), 0xA5, dtype=torch.uint8, device="cuda")          # noqa: E731
    bad_codes = [torch.zeros(K, R, dtype=torch.int8, device="cuda"), torch.zeros(K, R + 1, dtype=torch.uint8, device="cuda"),
                 torch.zeros(K, R, dtype=torch.uint8), torch.zeros(R, K, dtype=torch.uint8, device="cuda").t()]
    bad_scales = [torch.zeros(K, nb, dtype=torch.float32, device="cuda"), torch.zeros(K, nb + 1, dtype=torch.uint8, device="cuda"),
                  torch.zeros(K, nb, dtype=torch.uint8), torch.zeros(nb, K, dtype=torch.uint8, device="cuda").t()]
    for bad in bad_codes:
        s = good_s()
        with pytest.raises(ops.Fp8qError):
            ops.mx_encode_t(x, E4M3, out=bad, scales_out=s)
        assert (s == 0xA5).all()
        c, s = torch.full((R, K), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((R, K // 32), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(ops.Fp8qError):
            ops.mx_encode_both(x, E4M3, out=c, scales_out=s, out_t=bad, scales_out_t=good_s())
        assert (c == 0xA5).all() and (s == 0xA5).all()
    for bad in bad_scales:
        c = good_c()
        with pytest.raises(ops.Fp8qError):
            ops.mx_encode_t(x, E4M3, out=c, scales_out=bad)
        assert (c == 0xA5).all()
        c = good_c()
        with pytest.raises(ops.Fp8qError):
            ops.mx_encode_both(x, E4M3, out_t=c, scales_out_t=bad)
        assert (c == 0xA5).all()
    for bad in (torch.zeros(R, K, dtype=torch.float16, device="cuda"), torch.zeros(R, K + 1, device="cuda"), torch.zeros(R, K),
                torch.zeros(K, R, device="cuda").t()):
        with pytest.raises(ops.Fp8qError):
            ops.mx_quantize_t(x, E4M3, out=bad)
    with pytest.raises(ops.Fp8qError):
        ops.mx_quantize_t(x, E4M3, out_dtype=torch.bfloat16)
    # good ones are written in place, as views of the formats' dtypes
    c, s = good_c(), good_s()
    ct, st = ops.mx_encode_t(x, E4M3, out=c, scales_out=s)
    assert ct.data_ptr() == c.data_ptr() and st.data_ptr() == s.data_ptr() and ct.dtype == E4M3 and st.dtype == E8M0
    want = _ref(R, K, torch.float32, E4M3, "floor", True)
    _same(ct, want[0], "out=")
    _same(st, want[1], "scales_out=")
    y = torch.empty(R, K, device="cuda")
    assert ops.mx_quantize_t(x, E4M3, out=y).data_ptr() == y.data_ptr()
    _same(y, want[2].t(), "quantize_t out=")


def test_quantizer_with_blocks_along_dim_0():
    from fp8q import ops
    from quantization.mx import MXQuantizer
    torch.manual_seed(2)
    w = torch.randn(96, 72, device="cuda") * torch.logspace(-3, 3, 96, device="cuda").view(-1, 1)      # a block down a column spans magnitudes
    for fmt in (E4M3, E2M1, E3M2):
        q = MXQuantizer(fmt=fmt, rounding="ceil", block_axis=-2)
        y = q(w)
        assert torch.equal(y.view(torch.int32), ops.mx_quantize_t(w, fmt, "ceil").view(torch.int32))
        codes_t, scales_t = q.encode(w)
        assert tuple(scales_t.shape) == (72, 3) and codes_t.shape[0] == 72
        d = q.decode(codes_t, scales_t)
        assert tuple(d.shape) == (96, 72) and torch.equal(d.contiguous().view(torch.int32), y.view(torch.int32))
        _same(y, _oracle(w.cpu().t().contiguous(), fmt, "ceil")[2].t(), f"forward {_id[fmt]}")
        # block_axis=-1 is what it was
        q1 = MXQuantizer(fmt=fmt, rounding="ceil")
        assert torch.equal(q1(w).view(torch.int32), ops.mx_quantize(w, fmt, "ceil").view(torch.int32))
        assert not torch.equal(q1(w), y)                    # other blocks, other scales
    # a convolution weight through flatten_rows
    cw = torch.randn(8, 4, 3, 3, device="cuda")
    q = MXQuantizer(fmt=E4M3, block_axis=-2, flatten_rows=True)
    y = q(cw)
    assert y.shape == cw.shape
    _same(y, _oracle(cw.cpu().view(8, 36).t().contiguous(), E4M3, "floor")[2].t().reshape(8, 4, 3, 3), "conv weight")
    assert torch.equal(q.decode(*q.encode(cw)).contiguous().view(torch.int32), y.view(8, 36).view(torch.int32))
    with pytest.raises(ops.Fp8qError):
        MXQuantizer(fmt=E4M3, block_axis=-2)(cw)                           # not a matrix without flatten_rows
    q6 = MXQuantizer(fmt=E2M3, block_axis=-2, flatten_rows=True)
    assert q6(cw).shape == cw.shape                                        # shape[0] = 8
    with pytest.raises(ops.Fp8qError):
        q6(cw[:6].contiguous())                                            # shape[0] % 4 != 0
    with pytest.raises(ops.Fp8qError):
        q6.encode(cw[:6].contiguous())
    # keep_dtype on bfloat16
    xb = (torch.randn(64, 40, device="cuda") * 3).bfloat16()
    for keep in (False, True):
        q = MXQuantizer(fmt=E5M2, block_axis=-2, keep_dtype=keep)
        y = q(xb)
        dt = torch.bfloat16 if keep else torch.float32
        assert y.dtype == dt and y.shape == xb.shape
        _same(y, _oracle(xb.float().cpu().t().contiguous(), E5M2, "floor")[2].t().to(dt), f"keep_dtype={keep}")
        d = q.decode(*q.encode(xb), out_dtype=dt)
        assert torch.equal(d.contiguous().view(INT[dt]), y.view(INT[dt]))
