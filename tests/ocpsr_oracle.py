"""Stochastic rounding of the hardware FP8 lanes as the contract in include/fp8q.h reads, in torch CPU ops and written without
a look at the kernels: a helper of tests/test_ocpsr_host.py and tests/test_ocpsr_gpu.py, not a test module.

  codes_of        code = RNE(SR(q, r)): q = clamp(x / scale, -fmax, fmax) with torch's float32 division, SR by
                  mxsr_oracle.sr_round, the cast to torch.float8_* (exact on grid values), a NaN q as 0x7F; r=None: RNE(q)
  oracle          one scale per tensor or per row of x.view(C, -1): (codes, scale, values)
  oracle_block    one scale per (1, 128) / (128, 1) / (128, 128) tile, the geometry of tests/ocpb_oracle.py
  oracle_block_t  the transposed operands: oracle_block on x.t() with the draws of x, transposed
The draws are mxsr_oracle.draws(seed, offset, x.shape): by the flat index of the element in x as it lies.
"""
import torch

import mxsr_oracle as sro
from ocpb_oracle import FMAX, FMTS, same, bits          # noqa: F401  (re-exported for the tests)

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
NAME = {E4M3: "e4m3fn", E5M2: "e5m2"}
EPS = 1e-8


def codes_of(x, s, fmt, r=None):
    """uint8 codes of float32 x under float32 scales s (broadcastable); r: int64 draws shaped like x, or None for RNE"""
    fmax = FMAX[fmt]
    q = torch.clamp(x / s, -fmax, fmax)
    nan = torch.isnan(q)
    q = torch.where(nan, torch.zeros_like(q), q)
    if r is not None:
        q = sro.sr_round(q, r, fmt).view(q.shape)
    c = q.to(fmt).view(torch.uint8)
    return torch.where(nan, torch.tensor(0x7F, dtype=torch.uint8), c)


def _draws(seed, offset, shape, r):
    if r is not None or seed is None:
        return r
    return sro.draws(seed, offset, shape)


def oracle(x, maxval, fmt, eps=EPS, seed=None, offset=0, r=None):
    """(codes of dtype fmt, scale float32 [n], values float32); x float32 on the CPU, maxval float32 with 1 or x.shape[0]
    entries"""
    assert x.dtype == torch.float32 and fmt in FMAX
    maxval = maxval.reshape(-1).float()
    scale = torch.max(maxval, torch.tensor(eps, dtype=torch.float32)) / FMAX[fmt]
    s = scale.view((-1,) + (1,) * (x.dim() - 1)) if scale.numel() > 1 else scale
    c = codes_of(x, s, fmt, _draws(seed, offset, x.shape, r))
    return c.view(fmt), scale, c.view(fmt).float() * s


def oracle_block(x, fmt, tile, eps=EPS, seed=None, offset=0, r=None):
    """(codes, scales, values) under one scale per tile: ocpb_oracle.oracle's geometry"""
    tr, tk = tile
    x2 = x.reshape(-1, x.shape[-1])
    R, K = x2.shape
    Rp, Kp = -(-R // tr) * tr, -(-K // tk) * tk
    xp = torch.zeros(Rp, Kp)
    xp[:R, :K] = x2
    amax = xp.abs().view(Rp // tr, tr, Kp // tk, tk).amax(dim=(1, 3))
    scales = torch.max(amax, torch.tensor(eps, dtype=torch.float32)) / FMAX[fmt]
    s = scales.repeat_interleave(tr, 0).repeat_interleave(tk, 1)[:R, :K]
    r = _draws(seed, offset, x.shape, r)
    c = codes_of(x2, s, fmt, None if r is None else r.reshape(R, K)).view(fmt)
    sshape = tuple(x.shape[:-1]) + (Kp // tk,) if tr == 1 else (Rp // tr, Kp // tk)
    return c.view(x.shape), scales.view(sshape), (c.float() * s).view(x.shape)


def oracle_block_t(x, fmt, tile, eps=EPS, seed=None, offset=0):
    """the transposed operands of x [R, K]: the tile oracle on x.t() with x's draws transposed; everything is [K, R]-shaped"""
    r = None if seed is None else sro.draws(seed, offset, x.shape).t().contiguous()
    return oracle_block(x.t().contiguous(), fmt, tile, eps, r=r)
