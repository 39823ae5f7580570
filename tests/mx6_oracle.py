"""The 6-bit microscaling formats (E2M3 / E3M2 under an E8M0 block scale) as the contract in include/fp8q.h reads, in exact
torch CPU ops and written without a look at the kernels: a helper of tests/test_mx6_host.py and tests/test_mx6_gpu.py, not a
test module.

  scale byte   integer ops on the bits: m = the largest bits(|x|) of the zero-padded block of 32, E = m >> 23,
               man = m & 0x7fffff, code = max(E - emax + bump, 0), 0xFF when E == 255
  q            clamp(x * 2^(127 - code), -fmax, fmax) in float32, 2^n by bit construction
  element      e = max(exponent(|q|), emin) from the bits (emin = 1 - bias, the exponent of the smallest normal),
               step = 2^(e - M), r = torch.round(|q| / step) -- round half to even, and the division by a power of two is exact;
               the value is r * step, and the code follows from (e, r): r == 2^(M + 1) carries into the next binade,
               r >= 2^M is a normal with exponent field e + bias and mantissa r - 2^M, anything smaller is the subnormal r
  packing      four 6-bit codes in three bytes by integer shifts, element i of a row in bits [6i, 6i + 6)
  values       value(code) * X, one float32 multiplication; X = 2^(code - 127), code 0 the subnormal 0x00400000, 0xFF NaN
"""
import torch

E2M3, E3M2 = "e2m3", "e3m2"
FMTS = (E2M3, E3M2)
MBITS = {E2M3: 3, E3M2: 2}
BIAS = {E2M3: 1, E3M2: 3}
EMAX = {E2M3: 2, E3M2: 4}
FMAX = {E2M3: 7.5, E3M2: 28.0}
MAN_FMAX = {E2M3: 0x700000, E3M2: 0x600000}
BLOCK = 32


def pow2(n):
    """2^n as float32 by bit construction, n an int64 tensor in [-126, 127]"""
    return ((n + 127) << 23).to(torch.int32).view(torch.float32)


def scale_value(code):
    """X of a scale byte (int64 tensor)"""
    b = torch.where(code == 0, torch.tensor(0x00400000), torch.where(code == 255, torch.tensor(0x7FC00000), code << 23))
    return b.to(torch.int32).view(torch.float32)


def scale_code(m, fmt, rounding):
    """the scale byte (int64) of blocks whose largest bits(|x|) are m (int64)"""
    E, man = m >> 23, m & 0x7FFFFF
    bump = (man > MAN_FMAX[fmt]).long() if rounding == "ceil" else torch.zeros_like(E)
    code = torch.clamp(E - EMAX[fmt] + bump, min=0)
    return torch.where(E == 255, torch.tensor(255), code)


def element_codes(q, fmt):
    """(6-bit codes int64, magnitudes float32) of float32 q, finite and within +-fmax"""
    M, bias = MBITS[fmt], BIAS[fmt]
    emin = 1 - bias
    a = q.abs()
    e = torch.clamp(((a.view(torch.int32).long() >> 23) & 0xFF) - 127, min=emin)
    step = pow2(e - M)
    r = torch.round(a / step).long()
    mag = r.float() * step
    carry = r == (1 << (M + 1))
    e = torch.where(carry, e + 1, e)
    r = torch.where(carry, torch.tensor(1 << M), r)
    normal = r >= (1 << M)
    c = torch.where(normal, ((e + bias) << M) | (r - (1 << M)), r)
    assert int(c.max()) <= 31 and int(c.min()) >= 0
    sign = (q.view(torch.int32) < 0).long() << 5
    return c | sign, mag


def element_value(c, fmt):
    """the float32 value of 6-bit codes (int64), by the formulas of the contract"""
    M, bias = MBITS[fmt], BIAS[fmt]
    e, m = (c & 31) >> M, c & ((1 << M) - 1)
    sub = m.float() * (2.0 ** (1 - bias - M))
    nor = (1.0 + m.float() / (1 << M)) * pow2(torch.clamp(e - bias, min=-126))
    v = torch.where(e == 0, sub, nor)
    return torch.where((c & 32) != 0, -v, v)


def pack(c):
    """[..., K] 6-bit codes (int64, K % 4 == 0) -> uint8 [..., 3K / 4]"""
    K = c.shape[-1]
    assert K % 4 == 0
    g = c.reshape(c.shape[:-1] + (K // 4, 4))
    w = g[..., 0] | (g[..., 1] << 6) | (g[..., 2] << 12) | (g[..., 3] << 18)
    b = torch.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], -1)
    return b.reshape(c.shape[:-1] + (3 * K // 4,)).to(torch.uint8).contiguous()


def unpack(b):
    """uint8 [..., 3G] -> 6-bit codes int64 [..., 4G]"""
    n = b.shape[-1]
    assert n % 3 == 0
    t = b.long().reshape(b.shape[:-1] + (n // 3, 3))
    w = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)
    c = torch.stack([w & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 63], -1)
    return c.reshape(b.shape[:-1] + (4 * n // 3,))


def decode(codes, scales, fmt):
    """float32 values of packed codes (uint8 [..., 3K / 4]) under scale bytes (uint8 [..., ceil(K / 32)])"""
    c = unpack(codes)
    K = c.shape[-1]
    X = scale_value(scales.long()).repeat_interleave(BLOCK, -1)[..., :K]
    return (element_value(c, fmt) * X).contiguous()


def oracle(x, fmt, rounding):
    """(codes uint8 [..., 3K / 4], scales uint8 [..., ceil(K / 32)], values float32) of the contract; x float32 on the CPU,
    blocks along its last dimension, K % 4 == 0"""
    assert x.dtype == torch.float32 and not x.is_cuda and fmt in FMTS and rounding in ("floor", "ceil")
    lead, K = tuple(x.shape[:-1]), x.shape[-1]
    assert K % 4 == 0
    nb = (K + BLOCK - 1) // BLOCK
    xp = torch.zeros(lead + (nb * BLOCK,))
    xp[..., :K] = x
    xb = xp.view(lead + (nb, BLOCK))
    m = (xb.view(torch.int32) & 0x7FFFFFFF).amax(-1).long()           # non-negative int32: signed order == unsigned order
    code = scale_code(m, fmt, rounding)
    nanb = (code == 255).unsqueeze(-1)
    inv = pow2(torch.where(code == 255, torch.tensor(0), 127 - code)).unsqueeze(-1)
    q = torch.clamp(xb * inv, -FMAX[fmt], FMAX[fmt])
    q = torch.where(nanb, torch.zeros_like(q), q)
    c, _ = element_codes(q, fmt)
    c = torch.where(nanb, torch.tensor(0), c)
    vals = element_value(c, fmt) * scale_value(code).unsqueeze(-1)
    c = c.view(lead + (nb * BLOCK,))[..., :K]
    vals = vals.view(lead + (nb * BLOCK,))[..., :K].contiguous()
    return pack(c), code.to(torch.uint8), vals
