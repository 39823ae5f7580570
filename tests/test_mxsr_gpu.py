"""Stochastic rounding in the MX lane (seed= / offset= on ops.mx_encode, mx_quantize, mx_encode_t, mx_encode_both and
mx_quantize_t, MXQuantizer(stochastic=True)) against the oracle of tests/mxsr_oracle.py: torch integer ops on the CPU, as the
contract in include/fp8q.h reads.  Every comparison is on integers -- code bytes, scale bytes, the bit patterns of values with
every NaN mapped to one pattern -- and no element is left out.

Inputs are tests/test_mx_gpu.py's `_case` (magnitudes from 1e-44 to 1e38 with +-0, +-inf, NaN and a zero block).  Each
row-wise case runs four (seed, offset) pairs, rotated from case to case so that every one of the 16 pairs of the seeds 0, 1,
2^64 - 1, 0x0123456789ABCDEF and the offsets 0, 2^32 - 16 (the counter's low word wraps inside the tensor), 2^40 + 8 and
2^64 - 64 (the index wraps) is run many times over.  The transposed cases assert their route first."""
import functools

import pytest
import torch

import mxsr_oracle as sro
from mxsr_oracle import E2M1, E2M3, E3M2, E4M3, E5M2, FMTS, FP6, MULT, NAME
from test_mx_gpu import _case
from test_mxsr_host import FREQ, FREQ_SEEDS, freq_check, freq_input

pytestmark = pytest.mark.gpu

E8M0 = torch.float8_e8m0fnu
ROUNDINGS = ("floor", "ceil")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
HALVES = (torch.float16, torch.bfloat16)
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
SEEDS = (0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF)
OFFSETS = (0, 2 ** 32 - 16, 2 ** 40 + 8, 2 ** 64 - 64)
SHAPES = [(1, 32), (3, 64),                           # aligned
          (2, 31), (7, 33), (4, 148),                 # ragged (K trimmed to the format's divisibility)
          (3, 4128),                                  # rows that cross the 4096-element chunk of the vector route
          (2, 3, 8, 64)]                              # n-D
_dt = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}


def _ids(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return NAME.get(v) if isinstance(v, str) or v in NAME else _dt.get(v)


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


def _raw(t):
    """the bytes of a device tensor, for bit-for-bit identities between two results of the library"""
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype in (E4M3, E5M2, E2M1, E8M0) else t.view(INT[t.dtype])


def _equal(a, b):
    return a.shape == b.shape and torch.equal(_raw(a), _raw(b))


@functools.lru_cache(maxsize=None)
def _input(shape, fmt, dtype):
    K = shape[-1] // MULT[fmt] * MULT[fmt]
    return _case(shape)[..., :K].contiguous().to(dtype)


def _pairs(k):
    return [(SEEDS[i], OFFSETS[(i + k) % 4]) for i in range(4)]


# ---- row-wise: mx_encode and mx_quantize against the oracle ----
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rowwise_against_the_oracle(shape, fmt, rounding, dtype):
    from fp8q import ops
    x = _input(shape, fmt, dtype)
    xd = x.cuda()
    k = SHAPES.index(shape) + FMTS.index(fmt) + ROUNDINGS.index(rounding) + DTYPES.index(dtype)
    for seed, offset in _pairs(k):
        what = f"{shape} {NAME[fmt]} {rounding} {_dt[dtype]} seed {seed:#x} offset {offset:#x}"
        ref_c, ref_s, ref_y = sro.oracle(x.float(), fmt, rounding, seed, offset)
        codes, scales = ops.mx_encode(xd, fmt, rounding, seed=seed, offset=offset)
        assert codes.dtype == (torch.uint8 if fmt in FP6 else fmt) and scales.dtype == E8M0
        _same(scales, ref_s, f"{what}: scales")
        _same(codes, ref_c, f"{what}: codes")
        for dt in ([torch.float32] if dtype == torch.float32 else [torch.float32, dtype]):
            y = ops.mx_quantize(xd, fmt, rounding, out_dtype=dt, seed=seed, offset=offset)
            assert y.dtype == dt and y.shape == x.shape
            _same(y, ref_y.to(dt), f"{what}: quantize -> {dt}")
            d = ops.mx_decode(codes, scales, fmt=fmt if fmt in FP6 else None, out_dtype=dt)
            assert _equal(y, d), f"{what}: quantize != decode(encode) -> {dt}"


# ---- the transposed entries ----
def _t_cases():
    """(R, K, dtype, fmt): shapes that reach both kernels of mx_t_route and every width of the transposed code stores (the
    bytes of a codes_t row: R, R / 2 or 3R / 4), a short last tile in both directions (164 x 72), an odd K (general route)"""
    rows = {E4M3: (128, 36, 34), E5M2: (128, 36, 34), E2M1: (128, 40, 36), E2M3: (128, 48, 36), E3M2: (128, 48, 36)}
    out = []
    for fmt in FMTS:
        for R in rows[fmt]:
            out.append((R, 64, torch.float32, fmt))
        out.append((164, 72, torch.float32, fmt))
        out.append((164, 72, torch.float16, fmt))
        out.append((36, 72, torch.bfloat16, fmt))
        out.append((64, 33, torch.float32, fmt))             # general: K % 4 != 0
        out.append((36, 36, torch.bfloat16, fmt))            # general: a half type with K % 8 != 0
        out.append((40, 36, torch.float16, fmt))
    return out


T_CASES = _t_cases()
T_OFFSET = 2 ** 32 - 16


def _t_id(c):
    return f"{c[0]}x{c[1]}-{_dt[c[2]]}-{NAME[c[3]]}"


def _route(R, K, dtype):
    return "tile" if K % (4 if dtype == torch.float32 else 8) == 0 else "general"


def test_the_transposed_cases_reach_every_route_and_store_width():
    from fp8q import ops
    for fmt in FMTS:
        seen = set()
        for R, K, dtype, f in T_CASES:
            if f == fmt:
                r = ops.mx_t_route(R, K, fmt, dtype)
                assert r["kernel"] == _route(R, K, dtype)
                seen.add((r["kernel"], r["code_store_bytes"]))
                if R == 164:
                    assert R % r["tile_rows"] and K % r["tile_cols"] and R > r["tile_rows"] and K > r["tile_cols"]
        assert seen == {("tile", 16), ("tile", 4), ("tile", 1), ("general", 1)}, (NAME[fmt], seen)


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("case", T_CASES, ids=_t_id)
def test_transposed_against_the_oracle(case, rounding):
    from fp8q import ops
    R, K, dtype, fmt = case
    assert ops.mx_t_route(R, K, fmt, dtype)["kernel"] == _route(R, K, dtype)
    x = _case((K, R)).t().contiguous().to(dtype)           # the magnitude ladder runs across x's columns
    xd = x.cuda()
    fkw = dict(fmt=fmt) if fmt in FP6 else {}
    for seed, offset in ((SEEDS[3], T_OFFSET), (SEEDS[2], 0)):
        what = f"{R}x{K} {_dt[dtype]} {NAME[fmt]} {rounding} seed {seed:#x} offset {offset:#x}"
        tc, ts, ty = sro.oracle_t(x.float(), fmt, rounding, seed, offset)
        for dt in ([torch.float32] if dtype == torch.float32 else [torch.float32, dtype]):
            y = ops.mx_quantize_t(xd, fmt, rounding, out_dtype=dt, seed=seed, offset=offset)
            _same(y, ty.t().contiguous().to(dt), f"{what}: quantize_t -> {dt}")
        assert tc is not None                                # every R here packs into whole bytes
        codes_t, scales_t = ops.mx_encode_t(xd, fmt, rounding, seed=seed, offset=offset)
        _same(scales_t, ts, f"{what}: scales_t")
        _same(codes_t, tc, f"{what}: codes_t")
        assert _equal(ops.mx_decode(codes_t, scales_t, **fkw).t(), ops.mx_quantize_t(xd, fmt, rounding, seed=seed,
                                                                                     offset=offset))
        if K % MULT[fmt] == 0:
            rc, rs, _ = sro.oracle(x.float(), fmt, rounding, seed, offset)
            got = ops.mx_encode_both(xd, fmt, rounding, seed=seed, offset=offset)
            _same(got[0], rc, f"{what}: both, codes")
            _same(got[1], rs, f"{what}: both, scales")
            _same(got[2], tc, f"{what}: both, codes_t")
            _same(got[3], ts, f"{what}: both, scales_t")


# ---- identities, bit for bit ----
@functools.lru_cache(maxsize=None)
def _offgrid(R, K):
    """finite values of comparable size, none of them on a 4- to 8-bit grid"""
    g = torch.Generator().manual_seed(11)
    return (torch.randn(R, K, generator=g) * 3.0 + 0.001).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_identities(fmt, dtype):
    from fp8q import ops
    fkw = dict(fmt=fmt) if fmt in FP6 else {}
    x = _offgrid(136, 72).to(dtype).cuda()                    # tile route for both dtypes, a short last tile
    seed, offset = 0x0123456789ABCDEF, 2 ** 40 + 8
    kw = dict(seed=seed, offset=offset)
    enc = ops.mx_encode(x, fmt, **kw)
    # the same (seed, offset) gives the same bytes twice; another seed gives other bytes
    again = ops.mx_encode(x, fmt, **kw)
    assert _equal(enc[0], again[0]) and _equal(enc[1], again[1])
    other = ops.mx_encode(x, fmt, seed=seed + 1, offset=offset)
    assert _equal(enc[1], other[1]) and not _equal(enc[0], other[0])
    assert not _equal(enc[0], ops.mx_encode(x, fmt, seed=seed, offset=offset + 8)[0])
    assert not _equal(enc[0], ops.mx_encode(x, fmt)[0])
    # quantize == decode(encode), row-wise and transposed
    assert _equal(ops.mx_quantize(x, fmt, **kw), ops.mx_decode(*enc, **fkw))
    enc_t = ops.mx_encode_t(x, fmt, **kw)
    assert _equal(ops.mx_quantize_t(x, fmt, **kw), ops.mx_decode(*enc_t, **fkw).t())
    assert not _equal(enc_t[0], ops.mx_encode_t(x, fmt, seed=seed + 1, offset=offset)[0])
    # encode_both == (encode, encode_t)
    both = ops.mx_encode_both(x, fmt, **kw)
    assert _equal(both[0], enc[0]) and _equal(both[1], enc[1]) and _equal(both[2], enc_t[0]) and _equal(both[3], enc_t[1])
    # a slice encoded with the offset of its first element is the slice of the whole
    x16 = x[:16, :64].contiguous()
    whole = ops.mx_encode(x16, fmt, seed=seed, offset=offset)
    part = ops.mx_encode(x16[8:].contiguous(), fmt, seed=seed, offset=offset + 8 * 64)
    assert _equal(part[0], whole[0][8:]) and _equal(part[1], whole[1][8:])
    qpart = ops.mx_quantize(x16[8:].contiguous(), fmt, seed=seed, offset=offset + 8 * 64)
    assert _equal(qpart, ops.mx_quantize(x16, fmt, seed=seed, offset=offset)[8:])
    # grid points do not move: encoding what the operands decode to gives the codes back, with any seed
    rne = ops.mx_encode(x, fmt)
    values = ops.mx_decode(*rne, **fkw)
    for s in SEEDS:
        back = ops.mx_encode(values, fmt, seed=s)
        assert _equal(back[0], rne[0]) and _equal(back[1], rne[1]), s
        back_t = ops.mx_encode_t(ops.mx_decode(*ops.mx_encode_t(x, fmt), **fkw).t().contiguous(), fmt, seed=s, offset=64)
        assert _equal(back_t[0], ops.mx_encode_t(x, fmt)[0]), s
    # seed=None is a call without the keyword
    for op in (ops.mx_encode, ops.mx_quantize, ops.mx_encode_t, ops.mx_encode_both, ops.mx_quantize_t):
        a, b = op(x, fmt), op(x, fmt, seed=None, offset=0)
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        assert all(_equal(u, v) for u, v in zip(a, b)), op.__name__


# ---- the frequency of rounding away from zero ----
@pytest.mark.parametrize("fmt", list(FREQ), ids=[NAME[f] for f in FREQ])
def test_frequency_through_the_quantizer(fmt):
    """tests/test_mxsr_host.py's case and bound, on the kernels: successive calls of one MXQuantizer(stochastic=True) draw the
    seeds the host test uses, each call equals the oracle of its seed and meets the bound, the calls differ from one another,
    and last_seed reproduces each of them"""
    from fp8q import ops
    from quantization.mx import MXQuantizer
    x = freq_input(fmt)
    xd = x.cuda()
    q = MXQuantizer(fmt=fmt, stochastic=True, seed=FREQ_SEEDS[0])
    ups = []
    for n, seed in enumerate(FREQ_SEEDS):
        with torch.no_grad():
            y = q(xd)
        assert q.last_seed == seed and q.calls == n + 1
        assert _equal(y, ops.mx_quantize(xd, fmt, seed=q.last_seed))
        _same(y, sro.oracle(x, fmt, "floor", seed=seed)[2], f"{NAME[fmt]} call {n}")
        ups.append(freq_check(y.cpu(), fmt, f"{NAME[fmt]} call {n} seed {seed}"))
    assert not torch.equal(ups[0], ups[1]) and not torch.equal(ups[1], ups[2]) and not torch.equal(ups[0], ups[2])
    # encode draws the next seed; the transposed orientation meets the same bound (x.t(): the pinning element heads each
    # block of 32 rows)
    codes, scales = q.encode(xd)
    assert q.last_seed == FREQ_SEEDS[-1] + 1 and q.calls == 4
    fkw = dict(fmt=fmt) if fmt in FP6 else {}
    assert _equal(ops.mx_decode(codes, scales, **fkw), ops.mx_quantize(xd, fmt, seed=q.last_seed))
    xt = x[:4096].t().contiguous().cuda()                      # [32, 4096]: blocks along dim 0
    qt = MXQuantizer(fmt=fmt, stochastic=True, seed=FREQ_SEEDS[0], block_axis=-2)
    with torch.no_grad():
        yt = qt(xt)
    _same(yt, sro.oracle_t(xt.cpu(), fmt, "floor", seed=FREQ_SEEDS[0])[2].t().contiguous(), f"{NAME[fmt]} block_axis=-2")
