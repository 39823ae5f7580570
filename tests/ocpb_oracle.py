"""The oracle of the tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block.hip; include/fp8q.h states the contract), on the CPU
with torch's own cast, and the integer comparison its tests use.  Shared by tests/test_ocpb_gpu.py; nothing here needs a GPU.

oracle(x, fmt, tile, eps): pad x with +0 to whole tiles, amax over the tile axes of |x| (torch.amax: a NaN wins, then an
infinity), scale = torch.max(amax, eps) / fmax, broadcast back and cropped; codes = clamp(x / s, -fmax, fmax) through torch's
cast with 0x7F wherever the clamped quotient is NaN (the contract keeps no NaN sign; torch's cast does); values = codes.float()
* s.  same(): bytes and bit patterns, every element, NaNs mapped to one pattern first (whose payload a CPU kernel leaves behind
is no property of this library)."""
import torch

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
