"""CPU-only checks of the MX lane's stochastic rounding (the fp8q_mxsr_* entries, seed= / offset= on the five ops,
MXQuantizer(stochastic=True)): the oracle of tests/mxsr_oracle.py against known answers and values written down by hand, the
header and the ctypes table, argument errors at the C ABI before any launch and in Python before the device check, the
quantizer's bookkeeping, and the frequency bound on the oracle alone (tests/test_mxsr_gpu.py asserts the same bound, with the
same seeds, on the kernels)."""
import ctypes
import math
import os
import re

import pytest
import torch

import mxsr_oracle as sro
from mxsr_oracle import E2M1, E2M3, E3M2, E4M3, E5M2, FMTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"fp8q_mxsr_encode_f32": 10, "fp8q_mxsr_encode_h16": 11, "fp8q_mxsr_quantize_f32": 9, "fp8q_mxsr_quantize_h16": 11,
         "fp8q_mxsr_encode_t_f32": 10, "fp8q_mxsr_encode_t_h16": 11, "fp8q_mxsr_encode_both_f32": 12,
         "fp8q_mxsr_encode_both_h16": 13, "fp8q_mxsr_quantize_t_f32": 9, "fp8q_mxsr_quantize_t_h16": 11}
FLOOR, CEIL, F32, F16, BF16 = 0, 1, 0, 1, 2
_ids = [sro.NAME[f] for f in FMTS]

# ---- the frequency case, shared with tests/test_mxsr_gpu.py ----
FREQ_ROWS = 1 << 15
FREQ_SEEDS = (2024, 2025, 2026)                 # consecutive: MXQuantizer(stochastic=True, seed=2024) draws them call by call
# fmt: (the element that pins the scale byte to 127 = 2^emax, the value of the other 31, its lower neighbour, its upper one, p)
FREQ = {E2M1: (4.0, 2.25, 2.0, 3.0, 0.25),                          # a quarter up the step from 2 to 3
        E3M2: (16.0, 1.1875, 1.0, 1.25, 0.75),                      # three quarters up a normal step
        E4M3: (256.0, 2.5 * 2.0 ** -9, 2.0 ** -8, 3 * 2.0 ** -9, 0.5)}    # inside the subnormal range (below 2^-6, step 2^-9)


def freq_input(fmt):
    top, v, _, _, _ = FREQ[fmt]
    x = torch.full((FREQ_ROWS, 32), v, dtype=torch.float32)
    x[:, 0] = top
    return x


def freq_check(values, fmt, what):
    """values: float32 [FREQ_ROWS, 32] on the CPU.  Every element is one of the two neighbours and the share that went away
    from zero lies within 5 standard deviations of p: 5 * sqrt(p (1 - p) / N), N = 31 * 2^15 independent draws (0.0022 for
    p = 1/4) -- derived from the binomial law, not tuned; the 2^-16 granularity of p is far below it"""
    top, _, lo, hi, p = FREQ[fmt]
    body = values[:, 1:]
    assert (values[:, 0] == top).all(), what
    up = body == hi
    assert (up | (body == lo)).all(), f"{what}: a result that is neither neighbour"
    n = body.numel()
    share = up.sum().item() / n
    bound = 5 * math.sqrt(p * (1 - p) / n)
    print(f"{what}: share {share:.6f}, p {p}, bound {bound:.6f}")
    assert abs(share - p) <= bound, f"{what}: share {share} against p = {p} +- {bound}"
    return up


# ---- Philox and the draws ----
def _words(*w):
    return [int(v) for v in w]


def test_philox_known_answers():
    assert _words(*sro.philox(0, 0, 0, 0, 0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert _words(*sro.philox(f, f, f, f, f, f)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _words(*sro.philox(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # vectorised over the counter: the same words
    c0 = torch.tensor([0, 0xFFFFFFFF])
    out = sro.philox(c0, c0, c0, c0, c0, c0)
    assert [int(o[0]) for o in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(o[1]) for o in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def _draws_by_hand(seed, i):
    """the contract, element by element in Python integers"""
    g = (i >> 3) & ((1 << 61) - 1)
    out = _words(*sro.philox(g & 0xFFFFFFFF, g >> 32, 0, 0, seed & 0xFFFFFFFF, seed >> 32))
    return (out[(i >> 1) & 3] >> (16 * (i & 1))) & 0xFFFF


@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF])
def test_draws_follow_the_flat_index(seed):
    # the counter's low word wraps between two consecutive calls; the index itself wraps mod 2^64
    for offset in (0, 2 ** 32 - 16, 2 ** 35 - 8, 2 ** 40 + 8, 2 ** 64 - 16):
        r = sro.draws(seed, offset, (2, 16))
        want = [_draws_by_hand(seed, (offset + k) % 2 ** 64) for k in range(32)]
        assert r.flatten().tolist() == want, (seed, offset)
    # g = 2^32 - 1 and g = 2^32: the low counter word goes from ffffffff to 0 and the high one from 0 to 1
    r = sro.draws(seed, 2 ** 35 - 8, (16,))
    lo = _words(*sro.philox(0xFFFFFFFF, 0, 0, 0, seed & 0xFFFFFFFF, seed >> 32))
    hi = _words(*sro.philox(0, 1, 0, 0, seed & 0xFFFFFFFF, seed >> 32))
    assert r.tolist() == [(w >> s) & 0xFFFF for out in (lo, hi) for w in out for s in (0, 16)]
    # the draw belongs to the element: a slice that starts at flat index 8 * j draws what the whole draws there
    whole = sro.draws(seed, 64, (16, 64))
    assert torch.equal(sro.draws(seed, 64 + 8 * 64, (8, 64)), whole[8:])


# ---- SR(q, r) by hand ----
def _f(v):
    return torch.as_tensor(v, dtype=torch.float32).reshape(-1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sr(q, r, fmt):
    q = _f(q)
    return sro.sr_round(q, torch.full(q.shape, r, dtype=torch.int64), fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_sr_round_by_hand(fmt):
    M, B = sro.MBITS[fmt], sro.BIAS[fmt]
    g = sro.grid(fmt)
    assert g.numel() <= 2 ** 7 and g[-1].item() == sro.FMAX[fmt] and g[0].item() == 0.0
    assert g.numel() == {E4M3: 127, E5M2: 124, E2M1: 8, E2M3: 32, E3M2: 32}[fmt]
    one = 2.0 ** (1 - B)                              # the smallest normal
    step = 2.0 ** (1 - B - M)
    assert g[1].item() == step and g[1 << M].item() == one
    # grid points never move, under either extreme draw, with either sign; fmax stays fmax
    for r in (0, 1, 0x8000, 0xFFFF):
        for s in (1.0, -1.0):
            assert torch.equal(_bits(_sr(g * s, r, fmt)), _bits(g * s)), (r, s)
    assert _sr(sro.FMAX[fmt], 0xFFFF, fmt).item() == sro.FMAX[fmt] and _sr(-sro.FMAX[fmt], 0xFFFF, fmt).item() == -sro.FMAX[fmt]
    # between two neighbours: r = 0 truncates toward zero, whatever the fraction
    lo, hi = g[:-1], g[1:]
    inf = torch.tensor(float("inf"))
    for q in ((lo + hi) / 2, torch.nextafter(lo, inf), torch.nextafter(hi, -inf), lo + (hi - lo) * 0.25):
        assert ((q > lo) & (q < hi)).all()
        assert torch.equal(_sr(q, 0, fmt), lo) and torch.equal(_sr(-q, 0, fmt), -lo)
        # and the result is always one of the two neighbours
        for r in (1, 0x3FFF, 0x4000, 0x7FFF, 0x8000, 0xC000, 0xFFFF):
            y = _sr(q, r, fmt)
            assert ((y == lo) | (y == hi)).all(), r
    # r = 0xffff goes up exactly when f16 >= 1.  Normal range: f16 are the 16 bits under the kept mantissa
    nl, nh = lo[1 << M:], hi[1 << M:]
    sh = 23 - M
    f16_is_1 = (_bits(nl) + (1 << (sh - 16))).view(torch.float32)
    f16_is_0 = (_bits(nl) + ((1 << (sh - 16)) - 1)).view(torch.float32)          # every bit below f16 set
    assert torch.equal(_sr(f16_is_1, 0xFFFF, fmt), nh) and torch.equal(_sr(f16_is_1, 0xFFFE, fmt), nl)
    assert torch.equal(_sr(f16_is_0, 0xFFFF, fmt), nl)
    # the midpoint has f16 = 0x8000: up from r = 0x8000 on, P(up) = 1/2
    mid = (nl + nh) / 2
    assert torch.equal(_sr(mid, 0x8000, fmt), nh) and torch.equal(_sr(mid, 0x7FFF, fmt), nl)
    # format-subnormal range: |q| in units of 2^-16 of the step
    sl, shi = lo[:1 << M], hi[:1 << M]
    unit = step * 2.0 ** -16
    assert torch.equal(_sr(sl + unit, 0xFFFF, fmt), shi) and torch.equal(_sr(sl + unit, 0xFFFE, fmt), sl)
    assert torch.equal(_sr(sl + unit / 2, 0xFFFF, fmt), sl)
    q = sl + step * 0.25
    assert torch.equal(_sr(q, 0xC000, fmt), shi) and torch.equal(_sr(q, 0xBFFF, fmt), sl)
    # the border between the two ranges is crossed by a carry: the largest subnormal's neighbour is the smallest normal, and
    # the top of a binade carries into the exponent
    top_sub = one - step
    assert _sr(top_sub + step / 2, 0x8000, fmt).item() == one and _sr(top_sub + step / 2, 0x7FFF, fmt).item() == top_sub
    below2 = torch.nextafter(torch.tensor(2.0 * one), torch.tensor(0.0)).item()
    assert _sr(below2, 1, fmt).item() == 2.0 * one and _sr(below2, 0, fmt).item() == 2.0 * one - (one * 2.0 ** -M)
    # -0 and tiny negatives keep the sign on a zero result: the -0 codes
    tiny = torch.tensor([-0.0, -1e-45, -step * 2.0 ** -17])
    for r in (0, 0xFFFF):
        y = sro.sr_round(tiny, torch.full((3,), r, dtype=torch.int64), fmt)
        assert _bits(y).tolist() == [-2 ** 31] * 3, r
        c, v = sro.element(y, fmt)
        assert c.tolist() == [{E4M3: 0x80, E5M2: 0x80, E2M1: 8, E2M3: 0x20, E3M2: 0x20}[fmt]] * 3
    # the conversion after SR is exact: the element's value is SR's result
    q = torch.cat([(lo + hi) / 2, -(lo + hi) / 2])
    for r in (0, 0x8000, 0xFFFF):
        y = _sr(q, r, fmt)
        assert torch.equal(sro.element(y, fmt)[1], y)


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_oracle_without_a_seed_is_the_rne_oracle_and_with_one_stays_between_the_neighbours(fmt):
    import mx6_oracle as mx6
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 96, generator=g) * torch.logspace(-3, 3, 6).view(-1, 1)
    x[1, 3], x[2, 40], x[3, :32] = float("nan"), -0.0, 0.0
    c0, s0, v0 = sro.oracle(x, fmt, "floor")
    if fmt in sro.FP6:
        c6, s6, v6 = mx6.oracle(x, fmt, "floor")
        assert torch.equal(c0, c6) and torch.equal(s0, s6)
        assert torch.equal(torch.nan_to_num(v0, nan=7.0), torch.nan_to_num(v6, nan=7.0))
    c1, s1, v1 = sro.oracle(x, fmt, "floor", seed=3)
    assert torch.equal(s1, s0) and not torch.equal(c1, c0)
    # each value is the RNE value or its neighbour on the other side of x: never further than one step of the coarsest binade
    c2, _, v2 = sro.oracle(x, fmt, "floor", seed=4)
    assert not torch.equal(c2, c1)
    keep = ~torch.isnan(v0)
    assert torch.equal(torch.isnan(v1), ~keep)
    # a tensor on the grid does not move, whatever the seed
    cg, sg, vg = sro.oracle(torch.nan_to_num(v0, nan=1.0), fmt, "floor", seed=9)
    cr, sr_, vr = sro.oracle(torch.nan_to_num(v0, nan=1.0), fmt, "floor")
    assert torch.equal(cg, cr) and torch.equal(sg, sr_) and torch.equal(vg, vr)


# ---- the header, the ctypes table, the library ----
def test_header_declares_the_entries_and_keeps_the_version():
    text = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    for name, n in ARITY.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n, name
        assert args[-3:] == ["uint64_t seed", "uint64_t offset", "fp8q_stream_t stream"], name
        # the twin's list with the two arguments inserted before the stream
        twin = {"fp8q_mxsr_encode_t": "fp8q_mxt_encode", "fp8q_mxsr_encode_both": "fp8q_mxt_encode_both",
                "fp8q_mxsr_quantize_t": "fp8q_mxt_quantize", "fp8q_mxsr_encode": "fp8q_mx_encode",
                "fp8q_mxsr_quantize": "fp8q_mx_quantize"}[name[:-4]] + name[-4:]
        t = re.search(r"^int %s\(([^;]*)\);" % twin, text, re.M)
        targs = [a.strip() for a in t.group(1).split(",")]
        assert args[:-3] + args[-1:] == targs, (name, twin)
    assert len(set(re.findall(r"^int (fp8q_mxsr_\w+)\(", text, re.M))) == 10
    assert re.search(r"^#define FP8Q_VERSION 601\b", text, re.M)
    import fp8q
    assert fp8q.lib().fp8q_version() == 601


def test_lib_prototypes_match_the_header():
    import fp8q
    from fp8q import _lib, build
    twins = {"fp8q_mxsr_encode_t": "fp8q_mxt_encode", "fp8q_mxsr_encode_both": "fp8q_mxt_encode_both",
             "fp8q_mxsr_quantize_t": "fp8q_mxt_quantize", "fp8q_mxsr_encode": "fp8q_mx_encode",
             "fp8q_mxsr_quantize": "fp8q_mx_quantize"}
    for name, n in ARITY.items():
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        tres, targs = _lib.SIGNATURES[twins[name[:-4]] + name[-4:]]
        assert args == targs[:-1] + [ctypes.c_uint64, ctypes.c_uint64] + targs[-1:], name
        assert hasattr(fp8q.lib(), name)
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("fp8q_mxsr_")) == sorted(ARITY)
    # the draw and the rounding live in the shared header, which the build knows; the units define none of it
    hdr = open(os.path.join(build.CSRC, "fp8q_mxq.h")).read()
    assert "fp8q_mxq.h" in build.HEADERS
    for fn in ("philox4x32(", "mx_sr(", "mx_code4_sr("):
        assert re.search(r"^__device__ __forceinline__ \w+ %s" % re.escape(fn), hdr, re.M), fn
        for src in ("fp8q_mx.hip", "fp8q_mx_t.hip"):
            code = open(os.path.join(build.CSRC, src)).read()
            assert not re.search(r"^__device__ __forceinline__ \w+ %s" % re.escape(fn), code, re.M), (src, fn)


def test_c_abi_argument_errors_come_before_any_launch():
    import fp8q
    L = fp8q.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63             # never dereferenced: every call below is refused by the checks
    enc, ench, qnt, qnth = L.fp8q_mxsr_encode_f32, L.fp8q_mxsr_encode_h16, L.fp8q_mxsr_quantize_f32, L.fp8q_mxsr_quantize_h16
    enct, encth = L.fp8q_mxsr_encode_t_f32, L.fp8q_mxsr_encode_t_h16
    both, bothh = L.fp8q_mxsr_encode_both_f32, L.fp8q_mxsr_encode_both_h16
    qntt, qntth = L.fp8q_mxsr_quantize_t_f32, L.fp8q_mxsr_quantize_t_h16
    # an offset that is no multiple of 8, everything else in order
    for off in (1, 4, 7, 12, 2 ** 64 - 1, 2 ** 63 + 4):
        assert enc(p, p, p, 4, 32, 0, FLOOR, 5, off, None) == -1
        assert ench(p, p, p, BF16, 4, 32, 0, FLOOR, 5, off, None) == -1
        assert qnt(p, p, 4, 32, 0, FLOOR, 5, off, None) == -1
        assert qnth(p, p, F16, F16, 4, 32, 0, CEIL, 5, off, None) == -1
        assert enct(p, p, p, 4, 32, 0, FLOOR, 5, off, None) == -1
        assert encth(p, p, p, F16, 4, 32, 0, FLOOR, 5, off, None) == -1
        assert both(p, p, p, p, p, 4, 32, 0, FLOOR, 5, off, None) == -1
        assert bothh(p, p, p, p, p, BF16, 4, 32, 0, FLOOR, 5, off, None) == -1
        assert qntt(p, p, 4, 32, 0, FLOOR, 5, off, None) == -1
        assert qntth(p, p, BF16, BF16, 4, 32, 0, FLOOR, 5, off, None) == -1
    # a bad rounding
    for bad in (2, -1):
        assert enc(p, p, p, 4, 32, 0, bad, 5, 8, None) == -1 and qnt(p, p, 4, 32, 0, bad, 5, 8, None) == -1
        assert enct(p, p, p, 4, 32, 0, bad, 5, 8, None) == -1 and both(p, p, p, p, p, 4, 32, 0, bad, 5, 8, None) == -1
        assert qntth(p, p, BF16, BF16, 4, 32, 0, bad, 5, 8, None) == -1 and ench(p, p, p, F16, 4, 32, 0, bad, 5, 8, None) == -1
    # null pointers
    assert enc(None, p, p, 4, 32, 0, FLOOR, 5, 0, None) == -1 and enc(p, None, p, 4, 32, 0, FLOOR, 5, 0, None) == -1
    assert ench(p, p, None, BF16, 4, 32, 0, FLOOR, 5, 0, None) == -1
    assert qnt(None, p, 4, 32, 0, FLOOR, 5, 0, None) == -1 and qnth(p, None, F16, F16, 4, 32, 0, FLOOR, 5, 0, None) == -1
    assert enct(None, p, p, 4, 32, 0, FLOOR, 5, 0, None) == -1 and encth(p, None, p, F16, 4, 32, 0, FLOOR, 5, 0, None) == -1
    for i in range(5):
        a = [p] * 5
        a[i] = None
        assert both(*a, 4, 32, 0, FLOOR, 5, 0, None) == -1 and bothh(*a, F16, 4, 32, 0, FLOOR, 5, 0, None) == -1
    assert qntt(None, p, 4, 32, 0, FLOOR, 5, 0, None) == -1 and qntth(p, None, F16, F16, 4, 32, 0, FLOOR, 5, 0, None) == -1
    # the twin's other refusals, with its codes: formats, packing, types, shapes
    for bad in (3, 6, -1):
        assert enc(p, p, p, 4, 32, bad, FLOOR, 5, 0, None) == -2 and qntt(p, p, 4, 32, bad, FLOOR, 5, 0, None) == -2
    assert enc(p, p, p, 4, 33, 2, FLOOR, 5, 0, None) == -1 and enc(p, p, p, 4, 34, 4, FLOOR, 5, 0, None) == -1
    assert enct(p, p, p, 5, 32, 2, FLOOR, 5, 0, None) == -1 and both(p, p, p, p, p, 32, 6, 5, FLOOR, 5, 0, None) == -1
    assert ench(p, p, p, F32, 4, 32, 0, FLOOR, 5, 0, None) == -1 and qnth(p, p, F16, BF16, 4, 32, 0, FLOOR, 5, 0, None) == -1
    assert enc(p, p, p, 0, 32, 0, FLOOR, 5, 0, None) == -1 and qntt(p, p, 4, -1, 0, FLOOR, 5, 0, None) == -1
    assert enc(p + 2, p, p, 4, 32, 0, FLOOR, 5, 0, None) == -1


# ---- Python: the keywords ----
OPS = ("mx_encode", "mx_quantize", "mx_encode_t", "mx_encode_both", "mx_quantize_t")


@pytest.mark.parametrize("op", OPS)
def test_seed_and_offset_refusals_arrive_before_the_device_check(op):
    from fp8q import ops
    call = getattr(ops, op)
    x = torch.randn(32, 32)
    for bad in (True, False, 1.0, -1, 2 ** 64, torch.tensor(3), "7", (1,)):
        with pytest.raises(ops.Fp8qError, match="seed"):
            call(x, E4M3, seed=bad)
    for bad in (True, 8.0, -8, 2 ** 64, torch.tensor(8), "8"):
        with pytest.raises(ops.Fp8qError, match="offset"):
            call(x, E4M3, seed=1, offset=bad)
    for bad in (1, 4, 12, 2 ** 64 - 1):
        with pytest.raises(ops.Fp8qError, match="multiple of 8"):
            call(x, E4M3, seed=1, offset=bad)
    with pytest.raises(ops.Fp8qError, match="without a seed"):
        call(x, E4M3, offset=8)
    # keyword-only
    with pytest.raises(TypeError):
        call(x, E4M3, "floor", None, None, None, None, None, 5)
    # the rounding argument keeps its two values
    for bad in ("nearest", "up", None, "stochastic"):
        with pytest.raises(ops.Fp8qError, match="rounding"):
            call(x, E4M3, rounding=bad, seed=1)
    # well-formed calls get as far as the device check
    for kw in (dict(seed=0), dict(seed=2 ** 64 - 1, offset=2 ** 64 - 8), dict(seed=None), dict(seed=None, offset=0)):
        with pytest.raises(ops.Fp8qError, match="CUDA"):
            call(x, E4M3, **kw)


# ---- MXQuantizer ----
def test_quantizer_arguments_and_repr():
    from quantization.mx import MXQuantizer
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="stochastic"):
            MXQuantizer(stochastic=bad)
    for bad in (True, 1.0, -1, 2 ** 64, None, torch.tensor(1)):
        with pytest.raises(ValueError, match="seed"):
            MXQuantizer(stochastic=True, seed=bad)
        with pytest.raises(ValueError, match="seed"):
            MXQuantizer(seed=bad)
    q = MXQuantizer(fmt=E5M2, rounding="ceil")
    assert q.stochastic is False and q.seed == 0 and q.calls == 0 and q.last_seed is None
    assert "stochastic" not in q.extra_repr() and "seed" not in q.extra_repr()
    assert q.extra_repr().endswith("fmt=E5M2, rounding=ceil, flatten_rows=False, block_axis=-1")
    s = MXQuantizer(fmt=E5M2, rounding="ceil", stochastic=True, seed=77, block_axis=-2)
    assert s.extra_repr().endswith("fmt=E5M2, rounding=ceil, flatten_rows=False, stochastic=True, seed=77, block_axis=-2")
    # the forward-only rule stays
    with pytest.raises(NotImplementedError):
        s(torch.randn(32, 32, requires_grad=True))
    assert s.calls == 0
    from fp8q import ops
    with pytest.raises(ops.Fp8qError, match="CUDA"):
        s(torch.randn(32, 32))


def test_quantizer_bookkeeping(monkeypatch):
    from fp8q import ops
    from quantization.mx import MXQuantizer
    seen = []

    def fake(name):
        def op(x, fmt, rounding, **kw):
            seen.append((name, dict(kw)))
            return (x, x) if "encode" in name else x
        return op

    for name in ("mx_quantize", "mx_quantize_t", "mx_encode", "mx_encode_t"):
        monkeypatch.setattr(ops, name, fake(name))
    x = torch.randn(8, 32)
    q = MXQuantizer(stochastic=True, seed=2 ** 64 - 2)
    assert q.last_seed is None
    q(x)
    assert q.last_seed == 2 ** 64 - 2 and q.calls == 1
    q.encode(x)
    assert q.last_seed == 2 ** 64 - 1 and q.calls == 2
    q(x)
    assert q.last_seed == 0 and q.calls == 3                   # mod 2^64
    assert [(n, kw["seed"]) for n, kw in seen] == [("mx_quantize", 2 ** 64 - 2), ("mx_encode", 2 ** 64 - 1), ("mx_quantize", 0)]
    q.reseed(10)
    assert q.seed == 10 and q.calls == 0 and q.last_seed is None
    q(x)
    assert seen[-1] == ("mx_quantize", {"out_dtype": None, "seed": 10}) and q.last_seed == 10
    with pytest.raises(ValueError, match="seed"):
        q.reseed(-1)
    del seen[:]
    t = MXQuantizer(stochastic=True, seed=5, block_axis=-2)
    t(x)
    t.encode(x)
    assert [(n, kw["seed"]) for n, kw in seen] == [("mx_quantize_t", 5), ("mx_encode_t", 6)]
    # not stochastic: the ops are called as they always were, without the keyword, and nothing is counted
    del seen[:]
    d = MXQuantizer(seed=3)
    d(x)
    d.encode(x)
    assert seen == [("mx_quantize", {"out_dtype": None}), ("mx_encode", {})] and d.calls == 0 and d.last_seed is None


# ---- the frequency of rounding away from zero, on the oracle alone ----
@pytest.mark.parametrize("fmt", list(FREQ), ids=[sro.NAME[f] for f in FREQ])
def test_frequency_on_the_oracle(fmt):
    x = freq_input(fmt)
    ups = []
    for seed in FREQ_SEEDS:
        c, s, v = sro.oracle(x, fmt, "floor", seed=seed)
        assert (s == 127).all()
        ups.append(freq_check(v, fmt, f"{sro.NAME[fmt]} seed {seed}"))
    assert not torch.equal(ups[0], ups[1]) and not torch.equal(ups[1], ups[2])
