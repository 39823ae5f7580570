"""Stochastic rounding of the MX elements as the contract in include/fp8q.h reads, in torch integer ops on the CPU and written
without a look at the kernels: a helper of tests/test_mxsr_host.py and tests/test_mxsr_gpu.py, not a test module.

  philox      Philox4x32-10 on int64 tensors that hold 32-bit words; the 32 x 32 -> 64 bit products by 16-bit halves, so no
              intermediate passes 2^34
  draws       element i = offset + position mod 2^64 (carried in two 32-bit words): counter (g & 0xffffffff, g >> 32, 0, 0)
              with g = i >> 3, word (i >> 1) & 3, its low or high 16 bits by i & 1
  sr_round    SR(q, r) on the bits of |q|: the normal range by the integer carry, the format-subnormal range by one float32
              product, truncated; r is passed in explicitly
  oracle      the block logic of the MX contract (tests/mx6_oracle.py's, for all five formats) with elem = RNE(SR(q, r));
              the transposed operands are the row-wise oracle on x.t() with the draws transposed (`r=`)
"""
import torch

import mx6_oracle as mx6

E4M3, E5M2, E2M1, E2M3, E3M2 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2, "e2m3", "e3m2"
FMTS = (E4M3, E5M2, E2M1, E2M3, E3M2)
FP6 = (E2M3, E3M2)
MBITS = {E4M3: 3, E5M2: 2, E2M3: 3, E3M2: 2, E2M1: 1}
BIAS = {E4M3: 7, E5M2: 15, E2M3: 1, E3M2: 3, E2M1: 1}
EMAX = {E4M3: 8, E5M2: 15, E2M1: 2, E2M3: 2, E3M2: 4}
FMAX = {E4M3: 448.0, E5M2: 57344.0, E2M1: 6.0, E2M3: 7.5, E3M2: 28.0}
MAN_FMAX = {E4M3: 0x600000, E5M2: 0x600000, E2M1: 0x400000, E2M3: 0x700000, E3M2: 0x600000}
MULT = {E4M3: 1, E5M2: 1, E2M1: 2, E2M3: 4, E3M2: 4}           # elements that share whole bytes
NAME = {E4M3: "e4m3fn", E5M2: "e5m2", E2M1: "e2m1", E2M3: "e2m3", E3M2: "e3m2"}
FP4_VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
FP4_MIDS = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
BLOCK = 32
MASK = 0xFFFFFFFF


def _mulhilo(a, b):
    """(high, low) 32-bit words of a * b; a an int constant below 2^32, b an int64 tensor of 32-bit words"""
    ah, al = a >> 16, a & 0xFFFF
    bh, bl = b >> 16, b & 0xFFFF
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh              # each below 2^32
    mid = lh + hl + (ll >> 16)                                        # below 2^34
    return hh + (mid >> 16), ((mid & 0xFFFF) << 16) | (ll & 0xFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: four output words (int64 tensors of 32-bit words) of counter words c0..c3 and key words k0, k1"""
    c0, c1, c2, c3, k0, k1 = (torch.as_tensor(v, dtype=torch.int64) for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        h0, l0 = _mulhilo(0xD2511F53, c0)
        h1, l1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def draws(seed, offset, shape):
    """the 16-bit draws (int64, shaped `shape`) of a contiguous tensor whose first element has the flat index `offset`"""
    assert 0 <= seed < 1 << 64 and 0 <= offset < 1 << 64 and offset % 8 == 0
    n = 1
    for s in shape:
        n *= int(s)
    pos = torch.arange(n, dtype=torch.int64)
    lo = (offset & MASK) + (pos & MASK)                              # below 2^33
    hi = ((offset >> 32) + (pos >> 32) + (lo >> 32)) & MASK          # mod 2^64: the carry out of the high word is dropped
    lo = lo & MASK
    g_lo, g_hi = ((lo >> 3) | (hi << 29)) & MASK, hi >> 3
    out = torch.stack(philox(g_lo, g_hi, 0, 0, seed & MASK, seed >> 32), -1)
    w = out.gather(-1, ((lo >> 1) & 3).unsqueeze(-1)).squeeze(-1)
    return ((w >> (16 * (lo & 1))) & 0xFFFF).reshape(tuple(shape))


def sr_round(q, r, fmt):
    """SR(q, r): float32 on fmt's grid; q float32, finite and within +-fmax, r an int64 tensor of 16-bit draws"""
    M, B = MBITS[fmt], BIAS[fmt]
    sh = 23 - M
    bits = q.contiguous().view(torch.int32).long() & MASK
    a = bits & 0x7FFFFFFF
    f16 = (a >> (sh - 16)) & 0xFFFF
    nrm = ((a >> sh) + ((f16 + r) >> 16)) << sh
    u = (q.abs() * torch.tensor(2.0 ** (16 + B + M - 1), dtype=torch.float32)).floor().long()      # one float32 product
    n = (u + r) >> 16
    sub = (n.float() * torch.tensor(2.0 ** (1 - B - M), dtype=torch.float32)).view(torch.int32).long()
    mag = torch.where(a >= ((128 - B) << 23), nrm, sub)
    out = mag | (bits & 0x80000000)
    out = torch.where(out >= 1 << 31, out - (1 << 32), out)
    return out.to(torch.int32).view(torch.float32)


def grid(fmt):
    """the non-negative values of fmt's grid, ascending (float32)"""
    M, B = MBITS[fmt], BIAS[fmt]
    vals, e = [m * 2.0 ** (1 - B - M) for m in range(1 << M)], 1
    while True:
        for m in range(1 << M):
            v = (1 + m / (1 << M)) * 2.0 ** (e - B)
            if v > FMAX[fmt]:
                return torch.tensor(vals, dtype=torch.float32)
            vals.append(v)
        e += 1


def fp4_codes(q):
    a = q.abs()
    cnt = (a.unsqueeze(-1) > FP4_MIDS).sum(-1)
    tie = (a.unsqueeze(-1) == FP4_MIDS).any(-1) & (cnt % 2 == 1)
    return (cnt + tie.long()) | ((q.view(torch.int32) < 0).long() << 3)


def fp4_value(c):
    return FP4_VALUES[c & 7] * torch.where((c & 8) != 0, -1.0, 1.0)


def element(q, fmt):
    """(unpacked codes int64, values float32) of RNE(q) in fmt; q float32, finite and within +-fmax"""
    if fmt == E2M1:
        c = fp4_codes(q)
        return c, fp4_value(c)
    if fmt in FP6:
        c, _ = mx6.element_codes(q, fmt)
        return c, mx6.element_value(c, fmt)
    c = q.to(fmt).view(torch.uint8)
    return c.long(), c.view(fmt).float()


def oracle(x, fmt, rounding, seed=None, offset=0, r=None):
    """(codes uint8 or None, scales uint8 [..., ceil(K / 32)], values float32) of the contract; x float32 on the CPU, blocks
    along its last dimension.  seed=None and r=None: round to nearest even.  r: the draws shaped like x, instead of
    draws(seed, offset, x.shape).  codes are packed as the lane packs them ([..., K], [..., K / 2], [..., 3K / 4]); None where K
    does not pack into whole bytes."""
    assert x.dtype == torch.float32 and not x.is_cuda and fmt in FMTS and rounding in ("floor", "ceil")
    lead, K = tuple(x.shape[:-1]), x.shape[-1]
    nb = (K + BLOCK - 1) // BLOCK
    if r is None and seed is not None:
        r = draws(seed, offset, x.shape)
    xp = torch.zeros(lead + (nb * BLOCK,))
    xp[..., :K] = x
    xb = xp.view(lead + (nb, BLOCK))
    m = (xb.view(torch.int32) & 0x7FFFFFFF).amax(-1).long()           # non-negative int32: signed order == unsigned order
    E, man = m >> 23, m & 0x7FFFFF
    bump = (man > MAN_FMAX[fmt]).long() if rounding == "ceil" else torch.zeros_like(E)
    code = torch.where(E == 255, torch.tensor(255), torch.clamp(E - EMAX[fmt] + bump, min=0))
    nanb = (code == 255).unsqueeze(-1)
    inv = mx6.pow2(torch.where(code == 255, torch.tensor(0), 127 - code)).unsqueeze(-1)
    q = torch.clamp(xb * inv, -FMAX[fmt], FMAX[fmt])
    q = torch.where(nanb, torch.zeros_like(q), q)
    if r is not None:
        rp = torch.zeros(lead + (nb * BLOCK,), dtype=torch.int64)
        rp[..., :K] = r
        q = sr_round(q, rp.view(q.shape), fmt)
    c, v = element(q, fmt)
    X = mx6.scale_value(code).unsqueeze(-1)
    nan_code = 0x7F if fmt in (E4M3, E5M2) else 0
    c = torch.where(nanb, torch.tensor(nan_code), c)
    vals = torch.where(nanb, torch.full_like(v, float("nan")), v * X)
    c = c.view(lead + (nb * BLOCK,))[..., :K]
    vals = vals.view(lead + (nb * BLOCK,))[..., :K].contiguous()
    if K % MULT[fmt]:
        codes = None
    elif fmt == E2M1:
        codes = (c[..., 0::2] | (c[..., 1::2] << 4)).to(torch.uint8).contiguous()
    elif fmt in FP6:
        codes = mx6.pack(c)
    else:
        codes = c.to(torch.uint8).contiguous()
    return codes, code.to(torch.uint8), vals


def oracle_t(x, fmt, rounding, seed=None, offset=0):
    """the transposed operands of x [R, K]: the row-wise oracle on x.t() with x's draws transposed; values are [K, R]"""
    r = None if seed is None else draws(seed, offset, x.shape).t().contiguous()
    return oracle(x.t().contiguous(), fmt, rounding, r=r)
