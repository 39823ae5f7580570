"""The oracle of the tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block.hip; include/fp8q.h states the contract), on the CPU
with torch's own cast, and the integer comparison its tests use.  Shared by tests/test_ocpb_gpu.py; nothing here needs a GPU.

oracle(x, fmt, tile, eps): pad x with +0 to whole tiles, amax over the tile axes of |x| (torch.amax: a NaN wins, then an
infinity), scale = torch.max(amax, eps) / fmax, broadcast back and cropped; codes = clamp(x / s, -fmax, fmax) through torch's
cast with 0x7F wherever the clamped quotient is NaN (the contract keeps no NaN sign; torch's cast does); values = codes.float()
* s.  same(): bytes and bit patterns, every element, NaNs mapped to one pattern first (whose payload a CPU kernel leaves behind
is no property of this library)."""
import torch

ROW, COL, FULL = (1, 128), (128, 1), (128, 128)
FMTS = (torch.float8_e4m3fn, torch.float8_e5m2)
FMAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}
SUB = {torch.float8_e4m3fn: 2.0 ** -9, torch.float8_e5m2: 2.0 ** -16}      # smallest subnormal
EPS = 1e-8
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
TILES = ((1, 128), (128, 1), (128, 128))


def bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype in FMAX:
        return t.view(torch.uint8)
    if t.is_floating_point():
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    return t.view(INT[t.dtype])


def same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.shape} {g.dtype} != {w.shape} {w.dtype}"
    bad = (g != w).flatten().nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {g.numel()} differ, first at {bad[:5].tolist()}: " \
                             f"{g.flatten()[bad[:5]].tolist()} != {w.flatten()[bad[:5]].tolist()}"


def oracle(x, fmt, tile, eps=EPS):
    """(codes, scales, values) of the contract; x float32 on the CPU of any shape the op takes (a half input: x.float())"""
    tr, tk = tile
    fmax = FMAX[fmt]
    x2 = x.reshape(-1, x.shape[-1])
    R, K = x2.shape
    Rp, Kp = -(-R // tr) * tr, -(-K // tk) * tk
    xp = torch.zeros(Rp, Kp)
    xp[:R, :K] = x2
    amax = xp.abs().view(Rp // tr, tr, Kp // tk, tk).amax(dim=(1, 3))
    scales = torch.max(amax, torch.tensor(eps, dtype=torch.float32)) / fmax
    s = scales.repeat_interleave(tr, 0).repeat_interleave(tk, 1)[:R, :K]
    q = torch.clamp(x2 / s, -fmax, fmax)
    codes = torch.where(torch.isnan(q), torch.tensor(0x7F, dtype=torch.uint8), q.to(fmt).view(torch.uint8)).view(fmt)
    values = codes.float() * s
    sshape = tuple(x.shape[:-1]) + (Kp // tk,) if tr == 1 else (Rp // tr, Kp // tk)
    return codes.view(x.shape), scales.view(sshape), values.view(x.shape)


def case(shape, fmt, tile, seed=0):
    """x on the CPU: seeded normals times per-row magnitudes from 1e-6 to 1e4; in the first elements of the first, a middle
    and the last (edge) tile the special values of the per-tensor lane's tests -- +-0, +-inf, NaN, +-amax, the format's
    subnormal midpoints times the tile's scale, 1e-45 -- one group of them per tile, so that a tile keeps a finite range
    unless the group is the infinities' or the NaN's; and, with more than three tiles, one tile of zeros"""
    tr, tk = tile
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x2 = x.view(-1, shape[-1])
    R, K = x2.shape
    if R > 1:
        x2 *= torch.logspace(-6, 4, R).view(R, 1)
    nr, nk = -(-R // tr), -(-K // tk)
    tiles = [(i, j) for i in range(nr) for j in range(nk)]
    inf, nan, sub = float("inf"), float("nan"), SUB[fmt]

    def region(t):
        i, j = t
        return x2[i * tr:(i + 1) * tr, j * tk:(j + 1) * tk]

    def plant(t, vals):
        r = region(t)
        flat = r.reshape(-1).clone()
        k = min(flat.numel(), len(vals))
        flat[:k] = torch.tensor(vals[:k])
        r.copy_(flat.view(r.shape))

    def finite_group(t):
        r = region(t)
        mv = r.abs().max().item()
        s = max(mv, EPS) / FMAX[fmt]
        return [0.0, -0.0, mv, -mv, 0.4999 * sub * s, -0.4999 * sub * s, 0.5 * sub * s, -0.5001 * sub * s, 1e-45, -1e-45,
                1.5 * sub * s, -2.5 * sub * s, 0.75 * mv]

    picks = [tiles[0], tiles[len(tiles) // 2], tiles[-1]]
    plant(picks[0], finite_group(picks[0]))
    if len(tiles) > 1:
        plant(picks[-1], finite_group(picks[-1])[2:])          # the edge tile: +-amax first, it may hold a few elements only
    if len(tiles) > 2:
        plant(picks[1], [1.0, inf, -inf, -0.0, 0.0])           # scale = inf: finite -> +-0, infinities -> 0x7F
    if len(tiles) > 3:
        region(tiles[1]).zero_()                               # scale = eps / fmax, zero codes
        region(tiles[1])[0, 0] = -0.0
    if len(tiles) > 4:
        plant(tiles[2], [0.5, nan])                            # a NaN scale, every code 0x7F
    return x.contiguous()


# ---- inputs that take the redo of csrc/fp8q_ocpq.h, and the count of the elements that do ----------------------------------
# A code is made from x * fl(1/s) and redone by x / s where the two ends of the error interval disagree or the product is NaN.
# Seeded normals take that route about once in 2^16 elements; the tiles below take it in most of theirs.
HALF = (torch.float16, torch.bfloat16)
TIE_EPS = 1e-40         # below every range of tie_case, so that a tile's scale is its own amax / fmax (a subnormal eps)
TIE_KINDS = ("inexact 3.0", "exact", "overflow", "inexact 0.7", "large")


def tie_ranges(fmt, dtype):
    """the intended ranges m of tie_case's tiles, in the order of rotation (TIE_KINDS), each rounded to `dtype` (a tile's amax
    is a value of the tensor): 3.0 and 0.7 (1/s inexact), fmax * 2^-5 (s a power of two: 1/s and the ties exact), 1e-37 (s
    subnormal, 1/s overflows; float16 has no such value, its smallest subnormal 2^-24 stands there and overflows nothing) and
    3e38 (float16: 40960 = 5 * 2^13, which has values that take the redo under both formats; 6e4 has none under E5M2)"""
    f16 = dtype == torch.float16
    m = [3.0, FMAX[fmt] * 2.0 ** -5, 2.0 ** -24 if f16 else 1e-37, 0.7, 40960.0 if f16 else 3e38]
    return [torch.tensor(v, dtype=torch.float32).to(dtype).float().item() for v in m]


def tie_values(fmt, s):
    """V * s for the float32 scale s: the format's finite grid (+-0 once) times s, every midpoint of neighbouring grid values
    times s, and each such product's two float32 neighbours (the set of the per-tensor lane's test_every_midpoint_of_the_grid)
    -- 1009 values for E4M3FN, 985 for E5M2 -- in a fixed scattered order (a stride coprime to the count, a midpoint first),
    so that any run of 128 holds all four sorts and every magnitude"""
    g = torch.arange(256, dtype=torch.uint8).view(fmt).float()
    g = torch.unique(g[torch.isfinite(g)])
    mid = (g[:-1] + g[1:]) / 2 * s
    inf = torch.tensor(float("inf"))
    v = torch.cat([mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf), g * s])
    return v[(torch.arange(v.numel()) * 389) % v.numel()]


def _code(q, fmt):
    """the contract's code of a quotient: clamp, torch's cast, 0x7F for a NaN"""
    q = torch.clamp(q, -FMAX[fmt], FMAX[fmt])
    return torch.where(torch.isnan(q), torch.tensor(0x7F, dtype=torch.uint8), q.to(fmt).view(torch.uint8))


def _redo_masks(x, s, fmt):
    """(taken, wrong_without) of float32 x under float32 s (broadcastable), element by element: fp8q_ocpq.h's decision"""
    r = 1.0 / s
    r = torch.where(torch.isinf(r), torch.full_like(r, float("nan")), r)
    q0 = x * r
    taken = (_code(q0 * (1.0 - 2.0 ** -21), fmt) != _code(q0 * (1.0 + 2.0 ** -21), fmt)) | torch.isnan(q0)
    return taken, _code(q0, fmt) != _code(x / s, fmt)


_half_cache = {}


def half_search(fmt, dtype, m):
    """all 65536 patterns of a half dtype under the scale of range m: (values that take the redo or that the reciprocal alone
    gets wrong, the latter first, padded to 128 values at least with the patterns nearest to them; how many take the redo;
    how many the reciprocal alone gets wrong).  Empty where no pattern does either."""
    key = (fmt, dtype, m)
    if key not in _half_cache:
        allv = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).float()
        ok = torch.isfinite(allv) & (allv.abs() <= m)
        s = torch.tensor(m, dtype=torch.float32) / FMAX[fmt]
        taken, wrong = _redo_masks(allv, s, fmt)
        taken, wrong = taken & ok, wrong & ok
        first = torch.cat([wrong.nonzero().flatten(), (taken & ~wrong).nonzero().flatten()])
        picked, have = first.tolist(), set(first.tolist())
        d = 1
        while picked and len(picked) < 128 and d < 64:
            for p in first.tolist():
                for q in (p + d, p - d):
                    if 0 <= q < 65536 and ok[q] and q not in have:
                        have.add(q)
                        picked.append(q)
            d += 1
        _half_cache[key] = (allv[torch.tensor(picked, dtype=torch.long)], int(taken.sum()), int(wrong.sum()))
    return _half_cache[key]


def tie_kind_of_tiles(shape, tile, seed=0):
    """[tiles down, tiles across] int64: the index into TIE_KINDS / tie_ranges of every tile of tie_case(shape, ..., seed)"""
    R, K = 1, shape[-1]
    for d in shape[:-1]:
        R *= d
    nr, nk = -(-R // tile[0]), -(-K // tile[1])
    return (torch.arange(nr * nk).view(nr, nk) + seed) % len(TIE_KINDS)


def tie_case(shape, fmt, tile, dtype, seed=0):
    """x of `shape` and `dtype` on the CPU whose every tile is full of rounding ties under the tile's own scale.  Tile t (row
    major) has the range m = tie_ranges(fmt, dtype)[(t + seed) % 5] and holds V * s = tie_values(fmt, s), s = fl(m / fmax), from
    the offset 128 (t // 5 + seed) on (so the tiles of one range walk through V), clamped to [-m, m] and cast to dtype, after
    +m and -m, its first two elements: its amax is m exactly.  Edge tiles are filled by the same rule.  At (128, 1)
    neighbouring columns are neighbouring tiles, so the four columns of a lane have four different scales.  A half dtype
    rounds V * s off the ties, so its 3.0, 0.7 and 3e38 tiles hold half_search's values instead where there are any (the ties
    under a power-of-two scale are values of both half dtypes, and a 1e-37 tile is divided whatever it holds)."""
    tr, tk = tile
    x = torch.zeros(shape, dtype=dtype)
    x2 = x.view(-1, shape[-1])
    R, K = x2.shape
    kinds = tie_kind_of_tiles(shape, tile, seed)
    ranges = tie_ranges(fmt, dtype)
    for i in range(kinds.shape[0]):
        for j in range(kinds.shape[1]):
            r = x2[i * tr:(i + 1) * tr, j * tk:(j + 1) * tk]
            n, t = r.numel(), i * kinds.shape[1] + j
            kind = int(kinds[i, j])
            m = ranges[kind]
            src = tie_values(fmt, torch.tensor(m, dtype=torch.float32) / FMAX[fmt])
            if dtype in HALF and TIE_KINDS[kind] not in ("exact", "overflow") and half_search(fmt, dtype, m)[0].numel():
                src = half_search(fmt, dtype, m)[0]
            at = (torch.arange(n) - 2 + 128 * (t // len(TIE_KINDS) + seed)) % src.numel()    # (+m and -m take the first two places)
            fill = torch.clamp(src[at], -m, m)
            fill[:2] = torch.tensor([m, -m])[:n]
            r.copy_(fill.view(r.shape).to(dtype))
    return x


def redo_counts(x, fmt, tile, eps):
    """(taken, wrong_without), two int64 tensors [tiles down, tiles across] for x (float32 or half, on the CPU) under the
    oracle's scales: the elements of each tile that take the redo of fp8q_ocpq.h -- the codes of clamp(q0 (1 - 2^-21)) and
    clamp(q0 (1 + 2^-21)) differ or q0 is NaN, q0 = fl(x * fl(1/s)) with an infinite reciprocal replaced by NaN -- and those
    whose code from clamp(q0) alone is not the oracle's.  torch's CPU arithmetic, nothing of the library."""
    tr, tk = tile
    x2 = x.float().reshape(-1, x.shape[-1])
    R, K = x2.shape
    ref_c, scales, _ = oracle(x2, fmt, tile, eps)
    s2 = scales.view(-1, scales.shape[-1])
    s = s2.repeat_interleave(tr, 0).repeat_interleave(tk, 1)[:R, :K]
    taken, wrong = _redo_masks(x2, s, fmt)
    assert torch.equal(_code(x2 / s, fmt), ref_c.view(torch.uint8))
    nr, nk = s2.shape
    out = []
    for mask in (taken, wrong):
        p = torch.zeros(nr * tr, nk * tk, dtype=torch.int64)
        p[:R, :K] = mask
        out.append(p.view(nr, tr, nk, tk).sum(dim=(1, 3)))
    return out[0], out[1]


# the cases of tests/test_ocpb_ties_gpu.py, whose inputs tests/test_ocpb_host.py checks on the CPU.  Row-wise lane: (tile,
# shape, kernel) -- the smallest shapes that reach each kernel with more than one tile per reduction group: a wave's 8 tiles
# and a ninth row, more than one block's 32 tiles; panels ragged in both directions with K % 4 == 0, and whole ones; ragged K.
TIE_LANE_CASES = [(ROW, (9, 1024), "rows"), (ROW, (40, 256), "rows"), (ROW, (3, 130), "plain")] + \
                 [(t, s, k) for t in (COL, FULL) for s, k in (((136, 264), "panel"), ((256, 384), "panel"), ((130, 257), "plain"))]
# Transposed lane: shape -> (kernel, bytes per store of transposed codes), under (1, 128) and (128, 128)
TIE_T_SHAPES = {(144, 260): ("panel", 16), (132, 132): ("panel", 4), (130, 260): ("panel", 1), (129, 131): ("plain", 1)}
TIE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
