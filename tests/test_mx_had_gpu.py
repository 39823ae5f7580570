"""The block Hadamard rotation of the MX lane on the GPU (ops.hadamard32, hadamard= on mx_encode / mx_quantize / mx_encode_t /
mx_quantize_t, MXQuantizer(hadamard=)) against tests/test_mx_had_host.py's ten-line reference followed by the integer oracle of
tests/mxsr_oracle.py.  Codes and scales are compared byte for byte, values bit for bit with every NaN mapped to one pattern.

Shapes: [3, 64] the smallest; [5, 1024] a full 4096-element workgroup and a partial one (both branches of the quantize loop, the
dead lanes of encode); the same data through a view offset by one element (the general route); along dim 0 [160, 72], a full
128 x 64 tile and partial ones both ways, and [64, 67], the fallback.  Next to random normal blocks of mixed magnitude lie
constant blocks of +1.5 and -1.5 (their outputs 1 .. 31 are +0 under the contract, which -(b - a) would make -0), a block of
-0.0, one of zeros, one with an inf, one with a NaN, one of 3e38 whose sums overflow, and one with an outlier of 1e4."""
import functools

import pytest
import torch

import mxsr_oracle as sro
from fp8q import ops
from mxsr_oracle import E2M1, E2M3, E3M2, E4M3, E5M2
from test_mx_had_host import ref_had
from test_mxsr_gpu import _same

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CASES = [(d, f) for d in (F32, BF16, F16) for f in (E4M3, E2M1, E2M3)] + [(F32, E5M2), (F32, E3M2)]
IDS = [f"{str(d)[6:]}-{sro.NAME[f]}" for d, f in CASES]
ROW_SHAPES = ((3, 64), (5, 1024))
T_SHAPES = ((160, 72), (64, 67))
SEED = 1234


def _masks(shape):
    return (0, 0xFFFFFFFF, 0x80000001, int(torch.randint(1 << 32, (1,), generator=torch.Generator().manual_seed(sum(shape)))))


@functools.lru_cache(maxsize=None)
def _data(shape, dtype):
    """[R, K] of `dtype` on the CPU, blocks along K: random normal blocks of mixed magnitude, the planted ones at odd places"""
    nb = shape[0] * shape[1] // 32
    g = torch.Generator().manual_seed(shape[0] * 4099 + shape[1])
    span = 10 if dtype == F16 else 20
    x = torch.randn(nb, 32, generator=g) * torch.exp2(torch.randint(-span, span, (nb, 1), generator=g).float())
    near1 = 1.0 + 0.1 * torch.randn(32, generator=g)
    near1[7] = 1e4
    planted = [torch.full((32,), 1.5), torch.full((32,), -1.5), torch.full((32,), -0.0), torch.zeros(32),
               x[0].clone().index_fill_(0, torch.tensor([5]), float("inf")),
               x[0].clone().index_fill_(0, torch.tensor([30]), float("nan")), torch.full((32,), 3e38), near1]
    for k, blk in zip(range(1, nb, 2), planted):
        x[k] = blk
    return x.reshape(shape).to(dtype)


def _views(shape, dtype):
    """the tensor on the GPU as it is and as a view of a buffer one element in (no 16-byte alignment: the general route)"""
    x = _data(shape, dtype)
    buf = torch.empty(x.numel() + 1, dtype=dtype, device="cuda")
    buf[1:] = x.flatten().cuda()
    return x, (x.cuda(), buf[1:].view(shape))


def _t_input(shape, dtype):
    """x [R, K] whose columns are _data's rows, and x^T on the CPU in float32"""
    T = _data((shape[1], shape[0]), dtype)
    return T.t().contiguous().cuda(), T.float()


@pytest.mark.parametrize("dtype", (F32, BF16, F16), ids=lambda d: str(d)[6:])
def test_hadamard32(dtype):
    for shape in ROW_SHAPES:
        x, views = _views(shape, dtype)
        for m in _masks(shape):
            for xg in views:
                _same(ops.hadamard32(xg, m), ref_had(x.float(), m), f"forward {shape} {m:#x}")
                _same(ops.hadamard32(xg, m, inverse=True), ref_had(x.float(), m, inverse=True), f"inverse {shape} {m:#x}")
            if dtype != F32:
                _same(ops.hadamard32(views[0].float(), m, inverse=True, out_dtype=dtype),
                      ref_had(x.float(), m, inverse=True).to(dtype), f"float32 to half {shape} {m:#x}")


@pytest.mark.parametrize("dtype,fmt", CASES, ids=IDS)
def test_rowwise(dtype, fmt):
    for shape in ROW_SHAPES:
        x, views = _views(shape, dtype)
        for m in _masks(shape):
            rot = ref_had(x.float(), m)
            for seed in (None, SEED):
                codes, scales, vals = sro.oracle(rot, fmt, "floor", seed=seed)
                want = ref_had(vals, m, inverse=True)
                for xg in views:
                    c, s = ops.mx_encode(xg, fmt, hadamard=m, seed=seed)
                    _same(c.view(torch.uint8), codes, f"codes {shape} {m:#x} {seed}")
                    _same(s.view(torch.uint8), scales, f"scales {shape} {m:#x} {seed}")
                    q = ops.mx_quantize(xg, fmt, hadamard=m, seed=seed)
                    _same(q, want, f"quantize {shape} {m:#x} {seed}")
                    _same(ops.hadamard32(ops.mx_decode(c, s, fmt=fmt), m, inverse=True), q, "decode, rotate back == quantize")
                    if dtype != F32:
                        _same(ops.mx_quantize(xg, fmt, hadamard=m, seed=seed, out_dtype=dtype), want.to(dtype), "half out")
            # a row slice encoded with the offset of its first element is the slice of the whole
            c, s = ops.mx_encode(views[0][1:], fmt, hadamard=m, seed=SEED, offset=shape[1])
            _same(c.view(torch.uint8), codes[1:], f"slice codes {shape} {m:#x}")
            _same(s.view(torch.uint8), scales[1:], f"slice scales {shape} {m:#x}")


@pytest.mark.parametrize("dtype,fmt", CASES, ids=IDS)
def test_dim0(dtype, fmt):
    for shape, kernel in zip(T_SHAPES, ("tile", "general")):
        assert ops.mx_t_route(*shape, fmt, dtype)["kernel"] == kernel
        xg, T = _t_input(shape, dtype)
        for m in _masks(shape):
            rot_t = ref_had(T, m).t().contiguous()              # [R, K]: oracle_t cuts its blocks along dim 0
            for seed in (None, SEED):
                codes, scales, vals = sro.oracle_t(rot_t, fmt, "floor", seed=seed)
                want = ref_had(vals, m, inverse=True).t()
                c, s = ops.mx_encode_t(xg, fmt, hadamard=m, seed=seed)
                _same(c.view(torch.uint8), codes, f"codes_t {shape} {m:#x} {seed}")
                _same(s.view(torch.uint8), scales, f"scales_t {shape} {m:#x} {seed}")
                _same(ops.mx_quantize_t(xg, fmt, hadamard=m, seed=seed), want, f"quantize_t {shape} {m:#x} {seed}")
                if dtype != F32:
                    _same(ops.mx_quantize_t(xg, fmt, hadamard=m, seed=seed, out_dtype=dtype), want.to(dtype), "half out")


@pytest.mark.parametrize("dtype,fmt", [CASES[i] for i in (0, 1, 2, 4, 8)], ids=[IDS[i] for i in (0, 1, 2, 4, 8)])
def test_quantizer_and_default(dtype, fmt):
    from quantization.mx import MXQuantizer
    x = _data((160, 64), dtype).cuda()
    m = _masks((160, 64))[3]
    for axis in (-1, -2):
        for kw in ({}, {"stochastic": True, "seed": 7}):
            q = MXQuantizer(fmt=fmt, block_axis=axis, hadamard=m, keep_dtype=True, **kw)
            with torch.no_grad():
                y = q(x)
                q.reseed(q.seed)
                _same(q.decode(*q.encode(x), out_dtype=y.dtype), y, f"decode(encode) == forward, axis {axis} {kw}")
    for op in (ops.mx_encode, ops.mx_quantize, ops.mx_encode_t, ops.mx_quantize_t):
        for kw in ({}, {"seed": SEED}):
            a, b = op(x, fmt, hadamard=None, **kw), op(x, fmt, **kw)
            for got, want in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                _same(got, want, f"hadamard=None is today's {op.__name__}")
