"""ops.int_matmul on the GPU against the exact integer product, with torch alone: T = (qa - za) @ (qb - zb)^T in float64 (exact:
|T| < 2^53), qa / qb the codes read as signed or unsigned per the flag, z = clamp(rint(zero_float), 0, 2^n - 1), then
y_ref = T.float() * (sa[:, None] * sb[None, :]) in float32 with s = max(delta, eps).  Every assertion is torch.equal.

Codes are hand-made random bytes over the full range of n_bits, deltas random and no powers of two, zero_float from values that
round (-3.4 -> 0 after the clamp, 100.3, 17.5 -> 18, 127.5 -> 128) and values that clamp (-3.4, 300.0; 127.5 at 4 bits).
Shapes: (1, 1, 1); (17, 15, 72) a tail shorter than a step, load width 8, N % 4 != 0; (65, 129, 200) a tail, two tile columns;
(129, 65, 384) three steps, both LDS buffers reused, two tile rows; (130, 130, 257) width 1, a one-byte tail; (3, 260, 132)
width 4, three tile columns.  An operand is (mode, per channel, n_bits), mode asym / symS (signed flag set) / symU."""
import functools

import pytest
import torch

from fp8q import Fp8qError, ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (17, 15, 72), (65, 129, 200), (129, 65, 384), (130, 130, 257), (3, 260, 132)]
KINDS = [(("asym", False, 8), ("symS", True, 8)), (("asym", True, 8), ("asym", True, 8)), (("symU", False, 8), ("symS", False, 8)),
         (("symS", False, 8), ("symS", True, 8)), (("asym", False, 8), ("asym", False, 8)), (("asym", True, 4), ("symS", True, 8))]
ZEROS = [-3.4, 127.5, 300.0, 100.3, 17.5]
EPS = 1e-8


def _id(v):
    return "-".join("x".join(str(e) for e in t) if isinstance(t, tuple) else str(t) for t in v)


def _operand(rows, K, spec, seed, codes=None, delta=None, zero=None):
    """(keyword arguments of the operand without their prefix, q - z in float64 [rows, K], scale float32 [rows])"""
    mode, pc, n = spec
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-2 ** (n - 1), 2 ** (n - 1)) if mode == "symS" else (0, 2 ** n)
    q = torch.randint(lo, hi, (rows, K), generator=g) if codes is None else torch.full((rows, K), codes)
    nd = rows if pc else 1
    d = (torch.rand(nd, generator=g) * 0.05 + 0.011) if delta is None else delta
    kw = {"codes": (q & 255).to(torch.uint8).cuda(), "delta": d.cuda(), "n_bits": n, "symmetric": mode != "asym"}
    z = torch.zeros(nd, dtype=torch.float64)
    if mode == "asym":
        zf = torch.tensor([ZEROS[(seed + i) % len(ZEROS)] if zero is None else zero for i in range(nd)])
        kw["zero_float"] = zf.cuda()
        z = zf.round().clamp(0, 2 ** n - 1).double()
    else:
        kw["signed_flag"] = torch.tensor([mode == "symS"], dtype=torch.uint8).cuda()
    return kw, (q.double() - z[:, None]).cuda(), d.clamp(min=EPS).expand(rows).cuda()


@functools.lru_cache(maxsize=None)
def _pair(M, N, K, kinds):
    (ka, da, sa), (kb, db, sb) = _operand(M, K, kinds[0], 1), _operand(N, K, kinds[1], 2)
    return ka, kb, (da @ db.t()).float() * (sa[:, None] * sb[None, :])


def _mm(ka, kb, **kw):
    named = {f"{p}_{k}": v for p, o in (("a", ka), ("b", kb)) for k, v in o.items() if k not in ("codes", "delta")}
    return ops.int_matmul(ka["codes"], ka["delta"], kb["codes"], kb["delta"], eps=EPS, **named, **kw)


@pytest.mark.parametrize("kinds", KINDS, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_bit_equal(shape, kinds):
    ka, kb, ref = _pair(*shape, kinds)
    y = _mm(ka, kb)
    assert y.dtype == torch.float32 and torch.equal(y, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_half_out_and_leading_dimensions(dtype):
    ka, kb, ref = _pair(130, 129, 200, KINDS[4])
    y = _mm(dict(ka, codes=ka["codes"].view(2, 65, 200)), kb, out_dtype=dtype)
    assert y.shape == (2, 65, 129) and torch.equal(y.view(130, 129), ref.to(dtype))
    assert _mm(dict(ka, codes=ka["codes"][:0]), kb).shape == (0, 129)


@pytest.mark.parametrize("off", [1, 4, 8])
def test_operands_off_their_16_byte_alignment(off):
    ka, kb, ref = _pair(65, 129, 384, KINDS[0])

    def shifted(o):     # the same bytes, `off` bytes past a 16-byte boundary
        c = o["codes"]
        buf = torch.empty(c.numel() + 16, dtype=torch.uint8, device="cuda")
        buf[off:off + c.numel()] = c.flatten()
        return dict(o, codes=buf[off:off + c.numel()].view(c.shape))

    assert torch.equal(_mm(shifted(ka), shifted(kb)), ref)


@pytest.mark.parametrize("case", ["255x-255", "-255x-255", "random"])
def test_int32_edge(case):
    """K = 32768, the largest: |T| reaches 255^2 K = 2 130 739 200 with either sign, far past 2^24"""
    K, spec = 32768, ("asym", False, 8)
    fixed = {"255x-255": (255, 0.0), "-255x-255": (0, 255.0), "random": (None, None)}[case]
    ka, da, sa = _operand(16, K, spec, 1, codes=fixed[0], zero=fixed[1])
    kb, db, sb = _operand(16, K, spec, 2, codes=None if case == "random" else 0, zero=None if case == "random" else 300.0)
    T = da @ db.t()
    if case != "random":
        assert T.abs().min().item() == 2130739200 and (T < 0).all().item() == (case == "255x-255")
    assert torch.equal(_mm(ka, kb), T.float() * (sa[:, None] * sb[None, :]))
    with pytest.raises(Fp8qError, match="K must be in"):
        _mm(dict(ka, codes=torch.zeros(16, K + 1, dtype=torch.uint8).cuda()), dict(kb, codes=torch.zeros(16, K + 1, dtype=torch.uint8).cuda()))


def test_multiplies_what_int_decode_returns():
    """power-of-two deltas, K = 72: every product and sum is exact in float32, so y is the product of the decoded tensors"""
    ka, _, _ = _operand(17, 72, ("asym", False, 8), 1, delta=torch.tensor([2.0 ** -5]))
    kb, _, _ = _operand(15, 72, ("symS", True, 8), 2, delta=torch.exp2(-torch.arange(15.0) % 7))
    dec = [ops.int_decode(o["codes"], o["delta"], o.get("zero_float"), o.get("signed_flag"), 8, o["symmetric"], EPS).double()
           for o in (ka, kb)]
    assert torch.equal(_mm(ka, kb), (dec[0] @ dec[1].t()).float())
