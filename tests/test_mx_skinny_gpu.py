"""ops.mx_matmul(skinny=True) on the GPU against the float64 product of the operands' values.

Exact cases: the generator of tests/test_mx_mm_gpu.py (elements on the grid of all five formats, every block times 2^s, s in
{-1, 0, 1}): products are multiples of 2^-4 and |sum| <= 144 K < 2^20 for K <= 4096, 24 significant bits at most, so every
order of float32 summation -- any split -- gives the float64 product's bits.  (M, N, K, splits):
(1, 1, 32, None) one block, three lane groups and three waves idle; (16, 15, 96, None) no full step, N % 4 != 0;
(17, 65, 160, 2) MG = 2 with 15 rows masked, a second workgroup of one row, split 1 a one-block tail; (33, 64, 384, 1) MG = 4
with rows 33-63 masked, three steps on four waves; (64, 130, 640, None) five steps, the waves hold 2, 2, 1, 0;
(5, 129, 1056, 3) nine steps with a one-block tail, uneven splits; (16, 64, 1024, 8) one step per split, three idle waves in
every workgroup, the longest reduce.
Bound cases: Gaussian data with 1 % outliers times 50.  The factor is not measured on this kernel: 18480 is
tests/test_mx_mm_gpu.py's figure for the instruction on this data at this K, 2 (S + 2) the bound of the added float32
additions in units of 2^-24 * (|A| . |B|^T)."""
import functools

import pytest
import torch

from fp8q import Fp8qError, ops

pytestmark = pytest.mark.gpu

E4M3, E5M2, E2M1, E2M3, E3M2 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2, "e2m3", "e3m2"
PAIRS = [(f, f) for f in (E4M3, E5M2, E2M1, E2M3, E3M2)] + [(E4M3, E2M1), (E2M1, E5M2), (E2M3, E4M3), (E3M2, E2M1)]
SHAPES = [(1, 1, 32, None), (16, 15, 96, None), (17, 65, 160, 2), (33, 64, 384, 1), (64, 130, 640, None), (5, 129, 1056, 3),
          (16, 64, 1024, 8)]
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
    (M, N, K, splits), (fa, fb) = shape, pair
    a, ac, asc = _operand(M, K, fa, 1)
    b, bc, bsc = _operand(N, K, fb, 2)
    y = ops.mx_matmul(ac, asc, bc, bsc, skinny=True, splits=splits, **_fmt_kw(fa, fb))
    assert y.dtype == torch.float32 and torch.equal(y, (a @ b.t()).float())


@pytest.mark.parametrize("dtype, splits", [(torch.bfloat16, 2), (torch.float16, None)], ids=_id)
def test_exact_half_out_leading_dimensions_and_out(dtype, splits):
    a, ac, asc = _operand(34, 256, E4M3, 1)
    b, bc, bsc = _operand(130, 256, E2M3, 2)
    out = torch.empty(2, 17, 130, dtype=dtype, device="cuda")
    y = ops.mx_matmul(ac.view(2, 17, 256), asc.view(2, 17, 8), bc, bsc, b_fmt=E2M3, out_dtype=dtype, out=out, skinny=True,
                      splits=splits)
    assert y is out and torch.equal(y.view(34, 130), (a @ b.t()).to(dtype))


def test_workspace_of_the_caller():
    (M, N, K, splits), pair = (17, 65, 160, 2), (E4M3, E2M1)
    (a, ac, asc), (b, bc, bsc) = _operand(M, K, pair[0], 1), _operand(N, K, pair[1], 2)
    nbytes = ops.mx_skinny_plan(M, N, K, splits)[3]
    assert nbytes == 2 * M * N * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert torch.equal(ops.mx_matmul(ac, asc, bc, bsc, skinny=True, splits=splits, workspace=ws), (a @ b.t()).float())
    with pytest.raises(Fp8qError, match="workspace"):
        ops.mx_matmul(ac, asc, bc, bsc, skinny=True, splits=splits, workspace=ws[:nbytes - 16])


@pytest.mark.parametrize("off", [1, 4, 8])
@pytest.mark.parametrize("pair", [(E4M3, E2M1), (E2M3, E2M3)], ids=_id)
def test_exact_operands_off_their_16_byte_alignment(pair, off):
    (a, ac, asc), (b, bc, bsc) = _operand(17, 160, pair[0], 1), _operand(65, 160, pair[1], 2)

    def shifted(c):     # the same bytes, `off` bytes past a 16-byte boundary
        buf = torch.empty(c.numel() + 16, dtype=torch.uint8, device="cuda")
        buf[off:off + c.numel()] = c.view(torch.uint8).flatten()
        return buf[off:off + c.numel()].view(c.view(torch.uint8).shape)

    y = ops.mx_matmul(shifted(ac), asc, shifted(bc), bsc, a_fmt=pair[0], b_fmt=pair[1], skinny=True, splits=2)
    assert torch.equal(y, (a @ b.t()).float())


def test_exact_from_the_dim0_operands():
    """both operands from mx_encode_t of tensors that lie [K, rows]"""
    a, ac, asc = _operand(20, 96, E4M3, 3, t=True)
    b, bc, bsc = _operand(16, 96, E2M1, 4, t=True)
    assert torch.equal(ops.mx_matmul(ac, asc, bc, bsc, skinny=True), (a @ b.t()).float())


@pytest.mark.parametrize("pair", [(E4M3, E4M3), (E2M1, E2M1), (E2M3, E5M2)], ids=_id)
@pytest.mark.parametrize("shape", [(16, 129, 384, 2), (33, 65, 384, None)], ids=_id)
def test_summation_bound(shape, pair):
    (M, N, K, splits), (fa, fb) = shape, pair
    a, ac, asc = _operand(M, K, fa, 5, exact=False)
    b, bc, bsc = _operand(N, K, fb, 6, exact=False)
    y = ops.mx_matmul(ac, asc, bc, bsc, skinny=True, splits=splits, **_fmt_kw(fa, fb))
    S = ops.mx_skinny_plan(M, N, K, splits)[0]
    err, mag = (y.double() - a @ b.t()).abs(), a.abs() @ b.abs().t()
    print(f"S = {S}; largest error / (2^-24 * |A|.|B|^T): {(err / (2.0 ** -24 * mag)).max().item():.3f}")
    assert (err <= (18480 + 2 * (S + 2)) * 2.0 ** -24 * mag).all()
    assert torch.equal(ops.mx_matmul(ac, asc, bc, bsc, skinny=True, splits=splits, **_fmt_kw(fa, fb)), y)
