"""ops.ocp_block_matmul on the GPU against the float64 product of value(code) * scale, both taken in float64 and expanded by tile.

Exact cases: codes from {0, +-1, +-1.5, +-2, +-3, +-4, +-6} (exact in E4M3FN and E5M2), hand-made scales 2^s, s in {-1, 0, 1}, one
per tile.  Every term is a multiple of 2^-4 and sums stay below 36 * 4 * K <= 2^16 for K <= 384: every summation order gives the
same bits, so the result must EQUAL the float64 product, which proves the row, tile, byte and scale mapping and that the
unscaled instruction multiplies by 1.  Shapes: (1, 1, 128) a single tile; (17, 15, 72) a tail shorter than a step, load width 8,
N % 4 != 0; (65, 129, 200) width 8 with a tail; (129, 65, 384) three steps, both LDS buffers reused, three weight scale columns;
(130, 130, 257) width 1, 128-row scale tiles changing across workgroups; (3, 260, 132) width 4, three workgroup columns.
Bound cases: Gaussian data with 1 % outliers x 50 through the encoders (scales are no powers of two); |y - ref| <= F * 2^-24 *
(|A| . |B|^T) with decoded magnitudes.  Measured on exactly these cases: the largest ratio is 4628.965 (E4M3 x E4M3, the dW
form, K = 384; the other seven 2485.144 ... 3917.724); F is twice that.  mx_matmul's E4M3 x E4M3 figure on the same instruction
is 4298.054."""
import functools

import pytest
import torch

from fp8q import ops

pytestmark = pytest.mark.gpu

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
ROW, SQ = (1, 128), (128, 128)
TILES = [(ROW, SQ), (ROW, ROW), (SQ, SQ), (SQ, ROW)]
PAIRS = [(E4M3, E4M3), (E4M3, E5M2), (E5M2, E4M3), (E5M2, E5M2)]
SHAPES = [(1, 1, 128), (17, 15, 72), (65, 129, 200), (129, 65, 384), (130, 130, 257), (3, 260, 132)]
FACTOR = 9258       # twice the largest measured ratio of error to 2^-24 * (|A| . |B|^T) on the bound cases (4628.965)
GRID = torch.tensor([0.0, 1, 1.5, 2, 3, 4, 6, -1, -1.5, -2, -3, -4, -6])


def _id(v):
    return "x".join(str(e).replace("torch.float", "f").replace(" ", "") for e in (v if isinstance(v, tuple) else (v,)))


def _values(codes, scales, tile):
    """value(code) * scale in float64, the scales expanded over their tiles"""
    R, K = codes.shape
    s = scales.double().repeat_interleave(tile[0], 0)[:R].repeat_interleave(tile[1], 1)[:, :K]
    return codes.double() * s


@functools.lru_cache(maxsize=None)
def _exact(rows, K, fmt, tile, seed):
    """(values float64, codes, scales) on the GPU, hand-made: no encoder"""
    g = torch.Generator().manual_seed(seed)
    codes = GRID[torch.randint(len(GRID), (rows, K), generator=g)].cuda().to(fmt)
    scales = torch.exp2(torch.randint(-1, 2, (-(-rows // tile[0]), -(-K // 128)), generator=g).float()).cuda()
    return _values(codes, scales, tile), codes, scales


@functools.lru_cache(maxsize=None)
def _encoded(rows, K, fmt, tile, seed, t=False):
    """(values float64, codes, scales) from the encoders; t: made by ocp_block_encode_t from the [K, rows] tensor as it lies"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g)
    x[torch.rand(rows, K, generator=g) < 0.01] *= 50.0
    x = x.cuda()
    codes, scales = ops.ocp_block_encode_t(x.t().contiguous(), fmt, tile) if t else ops.ocp_block_encode(x, fmt, tile)
    return _values(codes, scales, tile), codes, scales


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
@pytest.mark.parametrize("tiles", TILES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_exact(shape, tiles, pair):
    (M, N, K), (ta, tb), (fa, fb) = shape, tiles, pair
    a, ac, asc = _exact(M, K, fa, ta, 1)
    b, bc, bsc = _exact(N, K, fb, tb, 2)
    y = ops.ocp_block_matmul(ac, asc, bc, bsc, ta, tb)
    assert y.dtype == torch.float32 and torch.equal(y, (a @ b.t()).float())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_id)
def test_exact_half_out_and_leading_dimensions(dtype):
    a, ac, asc = _exact(130, 200, E4M3, ROW, 1)
    b, bc, bsc = _exact(129, 200, E5M2, SQ, 2)
    y = ops.ocp_block_matmul(ac.view(2, 65, 200), asc.view(2, 65, 2), bc.view(torch.uint8), bsc, b_fmt=E5M2, out_dtype=dtype)
    assert y.shape == (2, 65, 129) and torch.equal(y.view(130, 129), (a @ b.t()).to(dtype))
    assert ops.ocp_block_matmul(ac[:0], asc[:0], bc, bsc).shape == (0, 129)


@pytest.mark.parametrize("off", [1, 4, 8])
def test_exact_operands_off_their_16_byte_alignment(off):
    (a, ac, asc), (b, bc, bsc) = _exact(65, 384, E4M3, ROW, 1), _exact(129, 384, E5M2, SQ, 2)

    def shifted(c):     # the same bytes, `off` bytes past a 16-byte boundary
        buf = torch.empty(c.numel() + 16, dtype=torch.uint8, device="cuda")
        buf[off:off + c.numel()] = c.view(torch.uint8).flatten()
        return buf[off:off + c.numel()].view(c.shape)

    y = ops.ocp_block_matmul(shifted(ac), asc, shifted(bc), bsc, a_fmt=E4M3, b_fmt=E5M2)
    assert torch.equal(y, (a @ b.t()).float())


@pytest.mark.parametrize("form", ["y", "dw"])
@pytest.mark.parametrize("pair", [(E4M3, E4M3), (E4M3, E5M2)], ids=_id)
@pytest.mark.parametrize("shape", [(65, 129, 200), (130, 130, 384)], ids=_id)
def test_summation_bound(shape, pair, form):
    (M, N, K), (fa, fb) = shape, pair
    ta, tb, t = (ROW, ROW, True) if form == "dw" else (ROW, SQ, False)
    a, ac, asc = _encoded(M, K, fa, ta, 5, t)
    b, bc, bsc = _encoded(N, K, fb, tb, 6, t)
    y = ops.ocp_block_matmul(ac, asc, bc, bsc, ta, tb).double()
    err, mag = (y - a @ b.t()).abs(), a.abs() @ b.abs().t()
    print(f"largest error / (2^-24 * |A|.|B|^T): {(err / (2.0 ** -24 * mag)).max().item():.3f}")
    assert (err <= FACTOR * 2.0 ** -24 * mag).all()
