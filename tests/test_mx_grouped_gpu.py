"""ops.mx_grouped_matmul on the GPU against the float64 product of each group's rows with that group's weights.

Operands, PAIRS and FACTOR are tests/test_mx_mm_gpu.py's; its docstring has the argument why the exact operands' sums are the
same bits in every summation order (K <= 384).  Group counts [0, 1, 33, 128, 0, 130, 0]: an empty first, middle and last group,
one row, one row past a 32-tile, exactly one 128-tile, a 128-tile plus two rows, and three padding rows (o_G = 292, T = 295).
N = 129: the tile edge and N % 4 != 0.  K = 160: a full step and a one-block tail; K = 384: three steps, both buffers reused;
K = 96 (one mixed pair): a single short step, the loop body run once with nothing in flight.
Bound cases: FACTOR is not measured on this kernel; it is the instruction's figure for the same chain of K steps.  The largest
ratio of error to 2^-24 * (|A| . |B|^T) measured, equal for both tile_m (the bits are mx_matmul's, which is asserted):
E4M3 x E4M3 5563.570, E2M1 x E2M1 0, E2M3 x E5M2 7286.073."""
import functools

import pytest
import torch

from fp8q import ops
from test_mx_mm_gpu import E2M1, E2M3, E4M3, E5M2, FACTOR, PAIRS, _fmt_kw, _id, _operand

pytestmark = pytest.mark.gpu

COUNTS, T, N = [0, 1, 33, 128, 0, 130, 0], 295, 129
G = len(COUNTS)
SENTINEL = -7.0


def _offsets(dtype=torch.int32, counts=COUNTS):
    return torch.tensor([0] + counts, dtype=torch.int64).cumsum(0).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _case(K, fa, fb, exact=True):
    """A's values / codes / scales, B's the same with B viewed [G, N, ...], and the float64 result with SENTINEL in the padding"""
    a, ac, asc = _operand(T, K, fa, 1 if exact else 5, exact)
    b, bc, bsc = _operand(G * N, K, fb, 2 if exact else 6, exact)
    ref, o = torch.full((T, N), SENTINEL, dtype=torch.float64, device="cuda"), _offsets().tolist()
    for g in range(G):
        ref[o[g]:o[g + 1]] = a[o[g]:o[g + 1]] @ b[g * N:(g + 1) * N].t()
    return (a, ac, asc), (b, bc.view(G, N, -1), bsc.view(G, N, -1)), ref


@pytest.mark.parametrize("K,pair", [(K, p) for K in (160, 384) for p in PAIRS] + [(96, (E4M3, E2M1))], ids=_id)
@pytest.mark.parametrize("tile_m", [32, 128])
def test_exact(tile_m, K, pair):
    (_, ac, asc), (_, bc, bsc), ref = _case(K, *pair)
    for dtype in (torch.int32, torch.int64):
        out = torch.full((T, N), SENTINEL, device="cuda")
        y = ops.mx_grouped_matmul(ac, asc, bc, bsc, _offsets(dtype), out=out, tile_m=tile_m, **_fmt_kw(*pair))
        assert y is out and torch.equal(y, ref.float())     # the padding rows [292, 295) keep the sentinel


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_id)
@pytest.mark.parametrize("tile_m", [32, 128])
def test_exact_half_out_one_group_and_all_empty(tile_m, dtype):
    (a, ac, asc), (b, bc, bsc), ref = _case(160, E4M3, E2M3)
    out = torch.full((T, N), SENTINEL, dtype=dtype, device="cuda")
    ops.mx_grouped_matmul(ac, asc, bc, bsc, _offsets(), b_fmt=E2M3, out_dtype=dtype, out=out, tile_m=tile_m)
    assert torch.equal(out, ref.to(dtype))
    one = torch.tensor([0, T], dtype=torch.int32, device="cuda")        # G = 1, o_1 = T: mx_matmul's product
    y = ops.mx_grouped_matmul(ac, asc, bc[2:3], bsc[2:3], one, b_fmt=E2M3, out_dtype=dtype, tile_m=tile_m)
    assert torch.equal(y, (a @ b[2 * N:3 * N].t()).to(dtype))
    out.fill_(SENTINEL)
    ops.mx_grouped_matmul(ac, asc, bc, bsc, torch.zeros(G + 1, dtype=torch.int64, device="cuda"), b_fmt=E2M3, out_dtype=dtype,
                          out=out, tile_m=tile_m)
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("off", [1, 4, 8])
@pytest.mark.parametrize("tile_m", [32, 128])
def test_exact_weights_off_their_16_byte_alignment(tile_m, off):
    (_, ac, asc), (_, bc, bsc), ref = _case(160, E4M3, E2M1)
    buf = torch.empty(bc.numel() + 16, dtype=torch.uint8, device="cuda")
    buf[off:off + bc.numel()] = bc.view(torch.uint8).flatten()
    shifted = buf[off:off + bc.numel()].view(bc.view(torch.uint8).shape)
    out = torch.full((T, N), SENTINEL, device="cuda")
    ops.mx_grouped_matmul(ac, asc, shifted, bsc, _offsets(), b_fmt=E2M1, out=out, tile_m=tile_m)
    assert torch.equal(out, ref.float())


@pytest.mark.parametrize("pair", [(E4M3, E4M3), (E2M1, E2M1), (E2M3, E5M2)], ids=_id)
@pytest.mark.parametrize("tile_m", [32, 128])
def test_summation_bound_and_the_bits_of_mx_matmul(tile_m, pair):
    (a, ac, asc), (b, bc, bsc), ref = _case(384, *pair, exact=False)
    y = ops.mx_grouped_matmul(ac, asc, bc, bsc, _offsets(), tile_m=tile_m, **_fmt_kw(*pair))
    o, worst = _offsets().tolist(), 0.0
    for g in range(G):
        rows = slice(o[g], o[g + 1])
        err, mag = (y[rows].double() - ref[rows]).abs(), a[rows].abs() @ b[g * N:(g + 1) * N].abs().t()
        worst = max(worst, (err / (2.0 ** -24 * mag)).max().item() if err.numel() else 0.0)
        assert (err <= FACTOR * 2.0 ** -24 * mag).all()
        assert torch.equal(y[rows], ops.mx_matmul(ac[rows], asc[rows], bc[g], bsc[g], **_fmt_kw(*pair)))
    print(f"largest error / (2^-24 * |A|.|B|^T): {worst:.3f}")


@pytest.mark.parametrize("tile_m", [32, 128])
def test_offsets_outside_the_contract_stay_inside_the_operands(tile_m):
    """[0, 5, 3, 400, 2] at T = 8: the local clamp gives the groups the rows [0, 5), [5, 5), [3, 8), [8, 8) -- overlapping,
    decreasing and past T, every one of them inside [0, T).  Each tensor the kernels touch is followed by a guard region."""
    Tn, Gn, K, guard = 8, 4, 160, 4096
    (_, ac, asc), (_, bc, bsc) = _operand(Tn, K, E4M3, 1), _operand(Gn * N, K, E2M1, 2)

    def guarded(t, fill):
        buf = torch.full((t.numel() * t.element_size() + guard,), fill, dtype=torch.uint8, device="cuda")
        buf[:buf.numel() - guard] = t.contiguous().view(torch.uint8).flatten()
        return buf, buf[:buf.numel() - guard].view(t.dtype).view(t.shape)

    bufs = [guarded(t, 0xA5) for t in (ac, asc, bc.view(Gn, N, -1), bsc.view(Gn, N, -1),
                                       torch.tensor([0, 5, 3, 400, 2], dtype=torch.int32, device="cuda"),
                                       torch.full((Tn, N), SENTINEL, device="cuda"),
                                       torch.zeros(ops.mx_grouped_plan(Tn, N, K, Gn, tile_m)[2], dtype=torch.uint8, device="cuda"))]
    xa, xs, wb, wsc, off, out, ws = (v for _, v in bufs)
    y = ops.mx_grouped_matmul(xa, xs, wb, wsc, off, out=out, tile_m=tile_m, workspace=ws)
    torch.cuda.synchronize()
    assert all((buf[-guard:] == 0xA5).all() for buf, _ in bufs)
    assert (torch.isfinite(y) | (y == SENTINEL)).all()
