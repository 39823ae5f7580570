"""ops.mx_matmul on the GPU against the float64 product of the operands' values.

Exact cases: elements from {0, +-1, +-1.5, +-2, +-3, +-4, +-6} (on the grid of all five formats), every block of 32 times 2^s,
s in {-1, 0, 1}.  Products are multiples of 2^-4 and sums stay below 36 * 4 * K <= 2^16 for K <= 384, 20 significant bits: every
order of float32 summation gives the same bits, so the result must EQUAL the float64 product -- which proves the row, block and
byte mapping of both operands and of the result (a permutation of K inside a block, consistent in both operands, would hide in
an equal-format pair: hence the mixed pairs).  Shapes: (1, 1, 32) one block, three lane groups masked; (17, 15, 96) a K tail
with no full step, N % 4 != 0; (65, 129, 160) a full step and a one-block tail, tile edges; (129, 65, 384) three steps, both
LDS buffers reused; (130, 130, 256).  Bound cases: Gaussian data with outliers against the float64 product of the decoded
operands.  The bound K * 2^-23 * (|A| . |B|^T) of K float32 additions over exact products is NOT met: the instruction aligns the
products of a group of 8 consecutive K to the group's largest and drops what falls below its window (DESIGN.md section 8 has
the probes).  Measured on these shapes: the largest error is 9239.652 * 2^-24 * (|A| . |B|^T) (E2M3 x E5M2 at K = 384; E4M3 x
E4M3 4298.054 and 3762.074, E2M1 x E2M1 0); the factor below is twice the measured value."""
import functools

import pytest
import torch

from fp8q import ops

pytestmark = pytest.mark.gpu

E4M3, E5M2, E2M1, E2M3, E3M2 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2, "e2m3", "e3m2"
PAIRS = [(f, f) for f in (E4M3, E5M2, E2M1, E2M3, E3M2)] + [(E4M3, E2M1), (E2M1, E5M2), (E2M3, E4M3), (E3M2, E2M1)]
SHAPES = [(1, 1, 32), (17, 15, 96), (65, 129, 160), (129, 65, 384), (130, 130, 256)]
FACTOR = 18480     # twice the largest measured ratio of error to 2^-24 * (|A| . |B|^T) on the bound cases' shapes (9239.652)
GRID = torch.tensor([0.0, 1, 1.5, 2, 3, 4, 6, -1, -1.5, -2, -3, -4, -6])


def _id(v):
    return "x".join(str(e).replace("torch.float", "f") for e in (v if isinstance(v, tuple) else (v,)))


@functools.lru_cache(maxsize=None)
def _operand(rows, K, fmt, seed, exact=True, t=False):
    """(values float64 [rows, K], codes, scales) on the GPU; t: made by mx_encode_t from the [K, rows] tensor as it lies"""
    g = torch.Generator().manual_seed(seed)
    if exact:
        x = GRID[torch.randint(len(GRID), (rows, K // 32, 32), generator=g)]
        x = (x * torch.exp2(torch.randint(-1, 2, (rows, K // 32, 1), generator=g).float())).view(rows, K)
    else:
        x = torch.randn(rows, K, generator=g)
        x[torch.rand(rows, K, generator=g) < 0.01] *= 50.0
    x = x.cuda()
    codes, scales = ops.mx_encode_t(x.t().contiguous(), fmt) if t else ops.mx_encode(x, fmt)
    vals = ops.mx_decode(codes, scales, fmt=fmt if isinstance(fmt, str) else None)
    if exact:
        assert torch.equal(vals, x), "the exact inputs must survive mx_encode / mx_decode"
    return vals.double(), codes, scales


def _fmt_kw(fa, fb):
    return {"a_fmt": fa if isinstance(fa, str) else None, "b_fmt": fb if isinstance(fb, str) else None}


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_exact(shape, pair):
    (M, N, K), (fa, fb) = shape, pair
    a, ac, asc = _operand(M, K, fa, 1)
    b, bc, bsc = _operand(N, K, fb, 2)
    y = ops.mx_matmul(ac, asc, bc, bsc, **_fmt_kw(fa, fb))
    assert y.dtype == torch.float32 and torch.equal(y, (a @ b.t()).float())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_id)
def test_exact_half_out_and_leading_dimensions(dtype):
    a, ac, asc = _operand(130, 256, E4M3, 1)
    b, bc, bsc = _operand(130, 256, E2M3, 2)
    y = ops.mx_matmul(ac.view(2, 65, 256), asc.view(2, 65, 8), bc, bsc, b_fmt=E2M3, out_dtype=dtype)
    assert y.shape == (2, 65, 130) and torch.equal(y.view(130, 130), (a @ b.t()).to(dtype))
    assert ops.mx_matmul(ac[:0], asc[:0], bc, bsc, b_fmt=E2M3).shape == (0, 130)


@pytest.mark.parametrize("off", [1, 4, 8])
@pytest.mark.parametrize("pair", [(E4M3, E2M1), (E2M3, E2M3)], ids=_id)
def test_exact_operands_off_their_16_byte_alignment(pair, off):
    (a, ac, asc), (b, bc, bsc) = _operand(65, 160, pair[0], 1), _operand(129, 160, pair[1], 2)

    def shifted(c):     # the same bytes, `off` bytes past a 16-byte boundary
        buf = torch.empty(c.numel() + 16, dtype=torch.uint8, device="cuda")
        buf[off:off + c.numel()] = c.view(torch.uint8).flatten()
        return buf[off:off + c.numel()].view(c.view(torch.uint8).shape)

    y = ops.mx_matmul(shifted(ac), asc, shifted(bc), bsc, a_fmt=pair[0], b_fmt=pair[1])
    assert torch.equal(y, (a @ b.t()).float())


@pytest.mark.parametrize("pair", [(E4M3, E2M1), (E3M2, E3M2)], ids=_id)
def test_exact_dw_from_the_dim0_operands(pair):
    """dW[20, 16] = dy^T . x over 96 tokens: both operands from mx_encode_t of tensors that lie [tokens, features]"""
    a, ac, asc = _operand(20, 96, pair[0], 3, t=True)
    b, bc, bsc = _operand(16, 96, pair[1], 4, t=True)
    assert torch.equal(ops.mx_matmul(ac, asc, bc, bsc, **_fmt_kw(*pair)), (a @ b.t()).float())


@pytest.mark.parametrize("pair", [(E4M3, E4M3), (E2M1, E2M1), (E2M3, E5M2)], ids=_id)
@pytest.mark.parametrize("shape", [(65, 129, 160), (130, 130, 384)], ids=_id)
def test_summation_bound(shape, pair):
    (M, N, K), (fa, fb) = shape, pair
    a, ac, asc = _operand(M, K, fa, 5, exact=False)
    b, bc, bsc = _operand(N, K, fb, 6, exact=False)
    y = ops.mx_matmul(ac, asc, bc, bsc, **_fmt_kw(fa, fb)).double()
    err, mag = (y - a @ b.t()).abs(), a.abs() @ b.abs().t()
    print(f"largest error / (2^-24 * |A|.|B|^T): {(err / (2.0 ** -24 * mag)).max().item():.3f} (float32 summation: {2 * K})")
    assert (err <= FACTOR * 2.0 ** -24 * mag).all()
