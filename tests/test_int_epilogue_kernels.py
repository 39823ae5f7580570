"""The INT fused epilogue (csrc/fp8q_intepilogue.hip): BN + residual + ReLU/ReLU6 + the per-tensor uniform quantizer in one
launch, bit for bit (a) the two-launch composition int_quantize(affine_act(x)) and (b) the CPU eager chain -- the uniform
quantizer on the CPU with the same range, applied to the oracle's act(bn(x) + residual) -- on every branch of the dispatch.
Every comparison is on integer bit patterns; a NaN may differ in its sign only."""
import functools

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

EPS = 1e-8
# (use_bn, use_res, act): BN+ReLU, BN+res+ReLU, res+ReLU, BN+ReLU6, BN, none
EPILOGUES = [(True, False, 1), (True, True, 1), (False, True, 1), (True, False, 2), (True, False, 0), (False, False, 0)]
# name -> (symmetric, x_min, x_max): symmetric signed, symmetric unsigned (no negative minimum), asymmetric
QUANTIZERS = {"sym_signed": (True, -3.1, 4.2), "sym_unsigned": (True, 0.0, 4.2), "asym": (False, -1.3, 4.2)}
SMALL = [(2, 8, 7, 7), (4, 16, 14, 14),
         (2, 8, 5, 5),          # 16-byte groups that cross planes
         (3, 12, 1, 1),         # HW < 4 with BN: the staged kernel, one group per lane, the plane constants in LDS
         (16, 5000),            # the same, thousands of planes per piece
         (5, 2, 1, 2),          # the same with two planes per image: the staged kernel's plane constants in registers
         (64, 1000),
         (1, 4, 256, 256),      # planes longer than a piece (1 MiB: the one-group-per-lane kernel, as everything below 64 MiB)
         (3, 40, 33, 31)]       # several steps per workgroup, ragged end of the image
ONE_COMBINATION = [(70000, 4, 1, 1),      # more images than gridDim.y allows
                   (64, 64, 64, 64),      # 64 MiB: the nontemporal staged kernel, planes of a piece: constants in registers
                   (64, 257, 32, 32)]     # the same kernel with the plane constants in LDS and a ragged last piece per image
CASES = ([(s, e, 8) for s in SMALL for e in EPILOGUES] + [((4, 16, 14, 14), e, nb) for e in EPILOGUES for nb in (4, 16)]
         + [(s, (True, True, 1), 8) for s in ONE_COMBINATION])


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _same_nan(a, b):
    """equal bits where not NaN, NaN at the same places (the sign of a NaN is not part of the contract)"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return (a.shape == b.shape and torch.equal(a.isnan(), b.isnan())
            and torch.equal(_bits(a.nan_to_num(0.0)), _bits(b.nan_to_num(0.0))))


def _cpu_quantizer(sym, n_bits, xmin, xmax):
    from quantization.uniform import SymmetricUniformQuantizer, AsymmetricUniformQuantizer
    q = (SymmetricUniformQuantizer if sym else AsymmetricUniformQuantizer)(n_bits=n_bits)
    q.set_quant_range(torch.tensor(xmin), torch.tensor(xmax))
    return q


@functools.lru_cache(maxsize=1)
def _case(shape, epi, n_bits):
    """Inputs and the CPU reference t = act(bn(x) + residual) of one case, computed once and left unchanged: seeded normals
    x 2, the probes NaN / inf / -0 in the first elements, and in every 7th position an exact rounding tie (k + 0.5) * delta of
    one of the three quantizers -- placed in a channel whose BN constants are the identity (every even channel) and on a zero
    residual, so that the tie is still a tie behind the epilogue."""
    use_bn, use_res, act = epi
    rng = np.random.RandomState(shape[0] * 7 + shape[1] + act + n_bits)
    N, C = shape[0], shape[1]
    HW = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    x = (rng.randn(*shape) * 2).astype(np.float32)
    res = rng.randn(*shape).astype(np.float32) if use_res else None
    bn = None
    if use_bn:
        var = (rng.rand(C) + 0.5).astype(np.float32)
        invstd = (np.float32(1) / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
        bn = [rng.randn(C).astype(np.float32), invstd, (rng.rand(C) + 0.5).astype(np.float32), rng.randn(C).astype(np.float32)]
        bn[0][::2], bn[1][::2], bn[2][::2], bn[3][::2] = 0.0, 1.0, 1.0, 0.0          # identity on the even channels
    deltas = [float(_cpu_quantizer(s, n_bits, lo, hi)._delta) for s, lo, hi in QUANTIZERS.values()]
    idx = np.arange(7, x.size, 7)
    if use_bn:
        idx = idx[((idx // HW) % C) % 2 == 0]
    k = rng.randint(-20, 20, idx.size).astype(np.float32)
    d = np.asarray(deltas, np.float32)[np.arange(idx.size) % 3]
    xf = x.reshape(-1)
    xf[idx] = (k + np.float32(0.5)) * d
    if use_res:
        res.reshape(-1)[idx] = 0.0
    xf[:3] = [np.nan, np.inf, -0.0]
    t = oracle.c_affine_act(x, tuple(bn) if bn else None, res, act)
    if idx.size:   # the ties survived the epilogue (the activation cuts the negative ones, ReLU6 those above 6)
        keep = (k >= 0 if act else np.ones(idx.size, bool)) & (xf[idx] <= 6 if act == 2 else True)
        assert keep.any() or idx.size < 16
        assert np.array_equal(t.reshape(-1)[idx[keep]], xf[idx[keep]])
    return x, res, bn, t


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@pytest.mark.parametrize("shape,epi,n_bits", CASES)
def test_fused_int_epilogue_bit_exact(shape, epi, n_bits):
    from fp8q import ops
    use_bn, use_res, act = epi
    x, res, bn, t = _case(shape, epi, n_bits)
    xd, rd = _dev(x), _dev(res)
    assert ops.affine_act_supported(xd)
    ab = ops.bn_fold(tuple(_dev(b) for b in bn)) if use_bn else None
    td = ops.affine_act(xd, ab, rd, act)
    tc = torch.from_numpy(t)
    assert _same_nan(td, tc)
    for name, (sym, lo, hi) in QUANTIZERS.items():
        qc = _cpu_quantizer(sym, n_bits, lo, hi)
        mn, mx = torch.tensor(lo, device="cuda"), torch.tensor(hi, device="cuda")
        # (c) the range variant: the range it reports is the CPU set_quant_range, bit for bit ...
        yr, delta, zf, sg = ops.int_affine_act_range_quantize(xd, mn, mx, n_bits, sym, EPS, bn_ab=ab, residual=rd, act=act)
        assert torch.equal(_bits(delta), _bits(qc._delta)), name
        if sym:
            assert sg.dtype == torch.bool and bool(sg) == bool(qc._signed) == (name == "sym_signed")
        else:
            assert torch.equal(_bits(zf), _bits(qc._zero_float)), name
        # (a) ... and both variants equal the two-launch composition on that range
        want = ops.int_quantize(td, delta, zf, sg, n_bits, sym, EPS)
        assert _same_nan(yr, want), (name, "range")
        yf = ops.int_affine_act_quantize(xd, delta, zf, sg, n_bits, sym, EPS, bn_ab=ab, residual=rd, act=act)
        assert _same_nan(yf, want), (name, "fixed")
        # (b) the CPU eager chain
        assert _same_nan(yf, qc(tc)), (name, "cpu")
        if shape in ONE_COMBINATION:
            continue
        # (d) out= aliasing x, and aliasing the residual: the same bits
        xa = xd.clone()
        assert ops.int_affine_act_quantize(xa, delta, zf, sg, n_bits, sym, EPS, bn_ab=ab, residual=rd, act=act, out=xa) is xa
        assert _same_nan(xa, want), (name, "out is x")
        if use_res:
            ra = rd.clone()
            y, *_ = ops.int_affine_act_range_quantize(xd, mn, mx, n_bits, sym, EPS, bn_ab=ab, residual=ra, act=act, out=ra)
            assert y is ra and _same_nan(ra, want), (name, "out is residual")


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("xmin,xmax", [(float("nan"), 1.0), (0.0, 0.0), (0.25, 3.0), (-2.0, float("nan")), (-1e-30, 1e-30)])
def test_range_variant_edge_ranges(sym, xmin, xmax):
    """A NaN x_min (symmetric: unsigned), x_min == x_max == 0, a positive x_min, a NaN x_max, a range below eps: delta /
    zero_float / sign as the CPU set_quant_range gives them, y as the composition on the reported range."""
    from fp8q import ops
    epi = (True, True, 1)
    x, res, bn, _ = _case((2, 8, 7, 7), epi, 8)
    xd, rd = _dev(x), _dev(res)
    ab = ops.bn_fold(tuple(_dev(b) for b in bn))
    qc = _cpu_quantizer(sym, 8, xmin, xmax)
    buf = dict(delta=torch.full((), 7.0, device="cuda"))          # caller's buffers are written in place
    buf.update(signed_flag=torch.ones((), dtype=torch.bool, device="cuda")) if sym else buf.update(
        zero_float=torch.full((), 7.0, device="cuda"))
    y, delta, zf, sg = ops.int_affine_act_range_quantize(xd, torch.tensor(xmin, device="cuda"), torch.tensor(xmax, device="cuda"),
                                                         8, sym, EPS, bn_ab=ab, residual=rd, act=1, **buf)
    assert delta is buf["delta"] and _same_nan(delta, qc._delta)
    if sym:
        assert sg is buf["signed_flag"] and bool(sg) == bool(qc._signed)
    else:
        assert zf is buf["zero_float"] and _same_nan(zf, qc._zero_float)
    want = ops.int_quantize(ops.affine_act(xd, ab, rd, 1), delta, zf, sg, 8, sym, EPS)
    assert _same_nan(y, want)


def test_unsupported_shape_is_reported():
    import fp8q
    x = torch.randn(2, 3, 5, 5, device="cuda")          # C*HW = 75: not a multiple of 4
    one = torch.ones(1, device="cuda")
    assert not fp8q.ops.affine_act_supported(x)
    with pytest.raises(fp8q.Fp8qError, match="unsupported"):
        fp8q.ops.int_affine_act_quantize(x, one, one, None, 8, False, EPS)
    with pytest.raises(fp8q.Fp8qError, match="unsupported"):
        fp8q.ops.int_affine_act_range_quantize(x, -one, one, 8, True, EPS)
    with pytest.raises(fp8q.Fp8qError, match="unsupported"):
        fp8q.ops.int_affine_act_quantize(x.view(2, 75)[:, :72].contiguous(), one, one, None, 17, False, EPS)   # n_bits
