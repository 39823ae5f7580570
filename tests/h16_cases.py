"""Shared builders of the half lane's tests (tests/test_h16_routes_host.py, tests/test_h16_routes_gpu.py): the shapes of
csrc/fp8q_h16.hip with the kernel and launcher choices each must reach, found with the host-only route query (ops.h16_route), and
the inputs that carry the hand-picked hard values of tests/epilogue_cases.py to every row border in a 16-bit type.  A helper, not a
test module; numpy only, needs no GPU.

  keys      K1:      ("quantize", dtype, C, inner, fmt, per_channel, x_phase)        -> dict(kernel=, u=)
            min/max: ("minmax", dtype, C, inner, x_phase)                              -> dict(kernel=, lanes= / nsplit=)
            fused:   ("minmax_quantize", dtype, C, inner, fmt, x_phase)                -> [scan dict, K1 dict]
            dtype is "float16" / "bfloat16"; x_phase the first element's offset from a 16-byte boundary in elements (0..7).
            A K1 key is run with a float32 and with a half output (the YF32 instances), at the y phases the test names.
  data      16-bit patterns as numpy uint16; widen() is the exact float32 value.
  inputs    quant_input: every row has its own range (row_ranges: every degenerate range -- 0, inf, NaN, 1e-40, 3e38 -- between two
            plain rows, so that a group straddling the border mixes the exact path of one row with the table of the other).  The
            edge values of a row's range (epilogue_cases.edge_values) lie over its first and last elements and on both sides of
            every 2048-element chunk border: for each float32 edge value the two neighbours in the input type, rounded toward zero
            and away from it -- the value itself where the type holds it.
            The first plain ranges have an integer bias (the default range and a power-of-two multiple of it: a range that is a
            power of two ITSELF has the bias 2^E - 1 - k + log2(2 - 2^-M), no integer; 4.0 is in the list all the same), so the
            grid step is a power of two and the ties (k + 1/2) s have 2 k + 1 <= 2^(M+2) as their significand: exact in float16
            (11 bits) for every format, in bfloat16 (8 bits) for every tie of the formats up to M = 6 and for the low ties
            (k = 0, 1, 2) of all.
"""
from math import gcd

import numpy as np

import rows_cases as rc
from epilogue_cases import FORMATS, bias32, default_maxval, edge_values, fmt_me, is_plain, ties

DTYPES = ("float16", "bfloat16")
FMTS = list(FORMATS) + ([rc.NARROW] if rc.NARROW not in FORMATS else [])
E5M2, E4M3 = rc.E5M2, rc.E4M3
CHUNK = 2048                # elements of a U = 1 chunk (256 lanes x 8); U = 4: 8192
BORDER = 8
MI = 1 << 20
BIG = (1 << 23) + 8         # U = 4 from 2^20 groups on, whatever the head
SLAB = 65535
MM_INNER = (8, 31, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048)
CH_INNER = (2040, 2047, 2048, 2049, 2056)


# ---------------------------------------------------------------------------------------------------------------------------
# 16-bit types on numpy
# ---------------------------------------------------------------------------------------------------------------------------
def widen(u, dt):
    u = np.ascontiguousarray(u, np.uint16)
    if dt == "float16":
        return u.view(np.float16).astype(np.float32)
    return (u.astype(np.uint32) << 16).view(np.float32)


def nearest(x, dt):
    """float32 -> patterns, round to nearest even (what torch.Tensor.to(dtype) does)"""
    x = np.ascontiguousarray(x, np.float32)
    if dt == "float16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    b = x.view(np.uint32)
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7fc0), r)


def toward_and_away(v, dt):
    """(rtz, raz) patterns of float32 values: equal where the type holds the value exactly.  The patterns of one sign are ordered
    like the magnitudes, infinity last, so the neighbour away from zero is the next pattern."""
    v = np.ascontiguousarray(v, np.float32)
    n = nearest(v, dt)
    with np.errstate(invalid="ignore"):
        back, mag = np.abs(widen(n, dt)), np.abs(v)
        rtz = np.where(back > mag, n - 1, n).astype(np.uint16)
        raz = np.where(back < mag, n + 1, n).astype(np.uint16)
    nan = np.isnan(v)
    return np.where(nan, n, rtz), np.where(nan, n, raz)


def edge_patterns(fmt, rng, dt):
    """the edge values of one range in the input type: rtz and raz of each, in the list's order"""
    ev = edge_values(fmt[0], rng if is_plain(rng) else 1.0, fmt[2], fmt[1])
    lo, hi = toward_and_away(ev, dt)
    return np.stack([lo, hi], 1).reshape(-1)


def exact_ties(fmt, rng, dt):
    """the ties of a range that the type holds exactly, as float32"""
    t = np.array([v for _, _, v, _ in ties(fmt[0], rng, fmt[2], fmt[1])], np.float32)
    lo, hi = toward_and_away(t, dt)
    ok = (lo == hi) & np.isfinite(t) & (t > 0)
    return t[ok]


# ---------------------------------------------------------------------------------------------------------------------------
# ranges
# ---------------------------------------------------------------------------------------------------------------------------
def scaled_default(fmt):
    """the default range times a power of two at which the reference's float32 chain still returns an integer bias"""
    d = default_maxval(fmt)
    for j in (-3, -2, -4, -1, -5, 1, 2, 3):
        b = bias32(fmt, d * 2.0 ** j)
        if float(b).is_integer():
            return d * 2.0 ** j
    raise AssertionError("no scaled default range with an integer bias for %r" % (fmt,))


def plain_ranges(fmt):
    return [default_maxval(fmt), scaled_default(fmt), 4.0, 2.5, 0.7361, 0.0123]


def degenerate_ranges(fmt):
    out = [1e-40, 3e38, float("inf"), 0.0, float("nan")]
    if fmt_me(fmt)[1] == 7:
        out.append(1e-30)
    return out


def is_degenerate(v):
    return not is_plain(v) or v in (1e-40, 3e38, 1e-30)


def row_ranges(fmt, C, pc=True):
    """plain, degenerate, plain | plain, degenerate, plain | ...: each list in turn"""
    P, D = plain_ranges(fmt), degenerate_ranges(fmt)
    if not pc:
        return [P[0]] * C
    out, p, d = [], 0, 0
    for r in range(C):
        if r % 3 == 1:
            out.append(D[d % len(D)])
            d += 1
        else:
            out.append(P[p % len(P)])
            p += 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# K1 inputs
# ---------------------------------------------------------------------------------------------------------------------------
def quant_input(key, seed=0):
    """dict(x uint16 [C, inner], maxval float32 [C] or [1], ranges, placed bool [C * inner]) of a K1 key.  Normals of the row's
    range / 2.3 rounded to the type; then the row's edge patterns over its first and last elements -- rows of up to 16 elements
    are edge patterns throughout, rows of a tensor with few rows take the whole list -- each row continuing in the list where the
    last row of the same range stopped; then BORDER patterns on each side of every chunk border of the flat range (counted from
    x's first 16-byte boundary, where the kernel's chunks start).  A per-tensor tensor is planted as rows of 509 elements."""
    _, dt, C, inner, fmt, pc, xp = key
    n = C * inner
    rng = np.random.RandomState(seed + 7 * inner + C)
    Cp, ip = (C, inner) if pc else (max(1, n // 509), min(n, 509))
    rr = row_ranges(fmt, Cp, pc)
    uniq = []
    for v in rr:
        if not any(v is u or v == u for u in uniq):
            uniq.append(v)
    kidx = np.array([next(i for i, u in enumerate(uniq) if v is u or v == u) for v in rr])
    scale = np.array([v if (is_plain(v) and not is_degenerate(v)) else 1.0 for v in uniq], np.float32)
    x = np.zeros(n, np.uint16)
    body = rng.standard_normal(Cp * ip).astype(np.float32) * np.repeat(scale[kidx] / np.float32(2.3), ip)
    x[:Cp * ip] = nearest(body, dt)
    x[Cp * ip:] = nearest(rng.standard_normal(n - Cp * ip).astype(np.float32), dt)
    placed = np.zeros(n, bool)
    per_row = min(ip, 16 if Cp >= 400 else 600)
    a = (per_row + 1) // 2
    inside = np.concatenate([np.arange(a), np.arange(ip - (per_row - a), ip)]).astype(np.int64)
    lists = [edge_patterns(fmt, u, dt) for u in uniq]
    for k, L in enumerate(lists):
        rows = np.flatnonzero(kidx == k)
        if not rows.size:
            continue
        # (a stride one short of the count: a value meets another position of the group the next time round)
        idx = (np.arange(rows.size, dtype=np.int64)[:, None] * per_row + np.arange(per_row)[None, :] + np.arange(rows.size)[:, None] // max(1, L.size // per_row)) % L.size
        pos = rows[:, None] * ip + inside[None, :]
        x[pos.reshape(-1)] = L[idx.reshape(-1)]
        placed[pos.reshape(-1)] = True
    head = (8 - xp) % 8
    b = np.arange(head + CHUNK, n, CHUNK, dtype=np.int64)
    if b.size:
        off = np.arange(-BORDER, BORDER, dtype=np.int64)
        bpos = (b[:, None] + off[None, :]).reshape(-1)
        bpos = bpos[bpos < n]
        brow = np.minimum(bpos // ip, Cp - 1)
        for k, L in enumerate(lists):
            sel = kidx[brow] == k
            x[bpos[sel]] = L[(bpos[sel] * 5 + 3) % L.size]
        placed[bpos] = True
    mv = np.array(rr if pc else rr[:1], np.float32)
    return dict(x=x.reshape(C, inner), maxval=mv, ranges=rr, placed=placed)


def straddles(key):
    """(flat offset of the group, b) of every 16-byte group of a per-channel key that crosses a row border: b elements of the
    group belong to the first row"""
    _, _, C, inner, _, _, xp = key
    n = C * inner
    head = min((8 - xp) % 8, n)
    g = head + 8 * np.arange((n - head) // 8, dtype=np.int64)
    b = inner - g % inner
    return g[b < 8], b[b < 8]


def all_patterns(rows, inner):
    """[rows, inner] uint16 whose flat data is the 65536 patterns tiled, every tile rotated by another amount: a pattern meets
    several positions of a group (and of a row)"""
    n = rows * inner
    i = np.arange(n, dtype=np.int64)
    return ((i + (i >> 16) * 4099) & 0xffff).astype(np.uint16).reshape(rows, inner)


# ---------------------------------------------------------------------------------------------------------------------------
# min/max and fused inputs
# ---------------------------------------------------------------------------------------------------------------------------
def rows_input(dt, C, inner, fmt, op, seed=0):
    """the row kinds of rows_cases.case_input (plain rows with their planted extreme first or last, NaN, +-inf, zeros of both signs,
    one-sided, denormal rows) rounded to the type.  For min/max every third row then has a larger extreme in its last element --
    the scalar tail of k_h16_minmax_rows wherever inner % 8 != 0 -- and every NaN row a second NaN there.
    Returns (x uint16 [C, inner], kinds)."""
    case = rc.case_input((C, inner), fmt, op, seed)
    x = nearest(case["x"].reshape(-1), dt).reshape(C, inner)
    if op == "minmax":
        one = nearest(np.array([1.0], np.float32), dt)[0]
        for r, (kind, s) in enumerate(case["kinds"]):
            if kind == "nan":
                x[r, inner - 1] = 0x7fc0
            elif kind == "plain" and r % 3 == seed % 3:
                with np.errstate(over="ignore"):
                    big = nearest(np.array([3.0 * s], np.float32), dt)[0]
                x[r, inner - 1] = (big if np.isfinite(widen(np.array([big]), dt)[0]) else one) | (0x8000 if r % 2 else 0)
    return x, case["kinds"]


def slab_input(seed=5):
    """the one slab case: [SLAB + 3, 2049] bfloat16 from random 16-bit patterns without NaN, the extremes and one NaN row planted
    in the rows around the slab border"""
    C, inner = SLAB + 3, 2049
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 1 << 16, C * inner, dtype=np.uint16).reshape(C, inner)
    x &= 0xbfff                                            # the top exponent bit masked out: no NaN, no infinity, |x| < 2
    x[SLAB - 1, 2048] = 0x7f7f                            # the largest finite value, last element of the first slab
    x[SLAB, 0] = 0xff7f                                    # its negative, first element of the second slab
    x[SLAB + 1, 1000] = 0x7fc0                             # a NaN row
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------
def qroute(ops, key):
    _, dt, C, inner, fmt, pc, xp = key
    return ops.h16_route("quantize", C, inner, pc, *fmt, x_mod16=2 * xp)


def first_chunk_inner(ops, fmt):
    """the shortest per-channel row the chunk kernel takes (at U = 1)"""
    for inner in range(1, 400):
        r = ops.h16_route("quantize", 600, inner, True, *fmt)
        if r["kernel"] == "k_h16_quant":
            assert r["u"] == 1
            return inner
    raise AssertionError(fmt)


def _q(dt, C, inner, fmt=E4M3, pc=True, xp=0):
    return ("quantize", dt, C, inner, fmt, pc, xp)


def short_row_keys(ops, dt, fmt):
    """rows of 8..15 elements at the x phases that give every b (the group offsets in a row are head + 8 q mod inner: one residue
    class of gcd(8, inner)), the shortest row of the chunk kernel and the one below it"""
    i0 = first_chunk_inner(ops, fmt)
    S = {}
    for inner in sorted(set(range(8, 16)) | {i0 - 1, i0}):
        phases = range(gcd(8, inner)) if 8 <= inner <= 15 else (0, 3)
        for xp in phases:
            k = _q(dt, 600, inner, fmt, True, xp)
            S[k] = dict(kernel="k_h16_quant" if inner >= i0 else "k_h16_quant_rows", u=1 if inner >= i0 else 0)
    return S


def big_keys(ops):
    """the four cases of 8 Mi elements and more: (a) per tensor U = 4, (b) / (c) per channel U = 4 on both sides of the 8192-element
    chunk, (d) a short row whose tables send U back to 1"""
    fall = next(i for i in range(8, 400) if ops.h16_route("quantize", BIG // i + 1, i, True, *E5M2)["kernel"] == "k_h16_quant")
    r = ops.h16_route("quantize", BIG // fall + 1, fall, True, *E5M2)
    assert r["u"] == 1 and r["groups"] >= MI
    return {
        _q("float16", 1, BIG + 5, E4M3, False, 3): dict(kernel="k_h16_quant", u=4, rows_per_chunk=1),
        _q("bfloat16", BIG // 8191 + 1, 8191, E5M2, True, 1): dict(kernel="k_h16_quant", u=4, rows_per_chunk=3),
        _q("float16", BIG // 8193 + 1, 8193, E4M3, True, 5): dict(kernel="k_h16_quant", u=4, rows_per_chunk=2),
        _q("bfloat16", BIG // fall + 1, fall, E5M2, True, 7): dict(kernel="k_h16_quant", u=1),
    }


def k1_groups(ops):
    """{group name: {key: expectation}}: a group is one test id"""
    G = {}
    for dt in DTYPES:
        for fmt in FMTS:
            G["short-%s-%s" % (dt, "x".join(str(v) for v in fmt))] = short_row_keys(ops, dt, fmt)
        S = {}
        for i, inner in enumerate(CH_INNER):
            for xp in (0, 3):
                S[_q(dt, 3 + (i + xp) % 3, inner, (E4M3, E5M2)[i % 2], True, xp)] = dict(kernel="k_h16_quant", u=1)
        G["chunk-switch-%s" % dt] = S
        S = {}
        for t in range(8):          # every tail 0..7, per tensor and per channel
            S[_q(dt, 1, 77 + t, E4M3, False, 0)] = dict(kernel="k_h16_quant", u=1, tail=(77 + t) % 8)
            S[_q(dt, 7, 11 + t, E4M3, True, 2)] = dict(kernel="k_h16_quant", u=1, tail=(7 * (11 + t) - 6) % 8)
        for xp in range(8):         # tensors smaller than their head
            for n in range(1, 8):
                S[_q(dt, 1, n, E4M3, False, xp)] = dict(kernel="k_h16_quant", u=1, head=min(n, (8 - xp) % 8), groups=0)
                S[_q(dt, n + 1, 1, E5M2, True, xp)] = dict(kernel="k_h16_quant_rows")
        G["tails-%s" % dt] = S
    for k, v in big_keys(ops).items():
        G["big-%s-%dx%d" % (k[1], k[2], k[3])] = {k: v}
    return G


def phase_keys(dt):
    """one short-row and one long-row shape per dtype, run at x phases 0..7 x every y phase and in place at every phase"""
    return [_q(dt, 37, 11, E4M3), _q(dt, 3, 2049, E5M2)]


def with_phase(key, xp):
    return key[:6] + (xp,)


def minmax_keys(ops):
    S = {}
    for j, dt in enumerate(DTYPES):
        for i, inner in enumerate(MM_INNER):
            gs = 0
            while gs < 6 and (32 << gs) < inner:
                gs += 1
            S[("minmax", dt, 2 * (256 >> gs) + 3, inner, (i + j) % 8)] = dict(kernel="k_h16_minmax_rows", lanes=1 << gs)
        S[("minmax", dt, 5, 2049, 1)] = dict(kernel="k_h16_minmax_part", nsplit=1, grid_y=5)
        S[("minmax", dt, 1, 2048, 3)] = dict(kernel="k_h16_minmax_part")
        S[("minmax", dt, 1, 300, 0)] = dict(kernel="k_h16_minmax_part", nsplit=1)
        S[("minmax", dt, 1, 5, 1)] = dict(kernel="k_h16_minmax_part", nsplit=1)      # a row shorter than its head (7)
        S[("minmax", dt, 1, 70001, 5)] = dict(kernel="k_h16_minmax_part")              # split over several blocks
    return S


def fused_keys(ops):
    S = {}
    for j, dt in enumerate(DTYPES):
        for fmt in (E4M3, E5M2, rc.NARROW):
            i0 = first_chunk_inner(ops, fmt)
            for inner in sorted({8, 9, 12, 15, i0 - 1, i0, 147}):
                k1 = "k_h16_quant" if inner >= i0 else "k_h16_quant_rows"
                S[("minmax_quantize", dt, 48, inner, fmt, (inner + j) % 8)] = [dict(kernel="k_h16_minmax_rows"), dict(kernel=k1)]
        for i, inner in enumerate(CH_INNER):
            S[("minmax_quantize", dt, 16, inner, (E4M3, E5M2)[i % 2], i)] = [
                dict(kernel="k_h16_minmax_rows" if inner <= 2048 else "k_h16_minmax_part"), dict(kernel="k_h16_quant", u=1)]
        S[("minmax_quantize", dt, 1, 100, E4M3, 1)] = [dict(kernel="k_h16_minmax_part", nsplit=1), dict(kernel="k_h16_quant", u=1)]
    return S


def instances():
    """every kernel instance quant_launch_u / quant_launch / minmax_launch can emit short of the nontemporal ones, as
    (kernel, U, per_channel, float32 out, dtype); what does not apply is None"""
    V = set()
    for dt in DTYPES:
        for yf32 in (True, False):
            V.add(("k_h16_quant_rows", None, True, yf32, dt))
            for pc in (True, False):
                for u in (1, 4):
                    V.add(("k_h16_quant", u, pc, yf32, dt))
        V.add(("k_h16_minmax_rows", None, None, None, dt))
        V.add(("k_h16_minmax_part", None, None, None, dt))
    return V


# four cases of 8 Mi elements over both dtypes leave one (U = 4, per tensor) pair to a single dtype
BEYOND_THE_CAP = {("k_h16_quant", 4, False, True, "bfloat16"), ("k_h16_quant", 4, False, False, "bfloat16")}
