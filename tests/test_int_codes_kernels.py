"""The integer codes of the uniform (INT) quantizers on the HIP kernels (csrc/fp8q_intcodec.hip): to_integer against the eager
torch chain (FP8Q_INT_KERNELS=0) on the same range buffers, encode against to_integer, decode(encode(x)) against int_quantize --
bit comparisons only --, the reference's recorded integers (tests/golden/gu2_uniform_int.npz), the kernel route actually taken,
no host synchronisation, and the symmetric sign read on the device.

Shapes are the CASES of tests/test_int_kernels.py (the same 4096-element chunking), each also through views that are not
co-aligned, so that the 16-byte paths and the element-wise path both run at either code width.  As that file's docstring
explains, the range buffers come from the CPU chain."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


class _NoSync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


class _Eager:
    """FP8Q_INT_KERNELS=0 for the duration: the reference's torch op chain on the same device"""
    def __enter__(self):
        self.prev = os.environ.get("FP8Q_INT_KERNELS")
        os.environ["FP8Q_INT_KERNELS"] = "0"

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop("FP8Q_INT_KERNELS", None)
        else:
            os.environ["FP8Q_INT_KERNELS"] = self.prev
        return False


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_nan(a, b):
    """equal bits where not NaN, NaN at the same places (the sign of a NaN is not part of the contract)"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and _same(a.nan_to_num(0.0), b.nan_to_num(0.0))


def _quantizer(sym, n_bits, per_channel):
    from quantization.uniform import SymmetricUniformQuantizer, AsymmetricUniformQuantizer
    return (SymmetricUniformQuantizer if sym else AsymmetricUniformQuantizer)(n_bits=n_bits, per_channel=per_channel)


def _with_buffers(q, dev):
    """a quantizer with copies of q's range buffers on `dev`"""
    qb = copy.deepcopy(q)
    qb._delta = q._delta.clone().to(dev)
    if q.symmetric:
        qb._signed = q._signed.clone().to(dev)
    else:
        qb._zero_float = q._zero_float.clone().to(dev)
    return qb


def _adversarial(shape, g):
    x = torch.randn(*shape, generator=g) * 3.0
    f = x.view(-1)
    n = f.numel()
    idx = torch.randperm(n, generator=g)
    k = max(n // 16, 1)
    f[idx[:k]] = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1e30, -1e30, float("inf"), float("-inf")]).repeat(k)[:k]
    return x


def _ties(x, q):
    """put exact rounding ties (k + 0.5) * delta of the quantizer's range into every 7th element"""
    d = q._delta.reshape(-1, *([1] * (x.dim() - 1))) if q._delta.dim() else q._delta
    k = torch.randint(-20, 20, x.shape, generator=torch.Generator().manual_seed(3)).float()
    t = ((k + 0.5) * d.cpu()).expand_as(x)
    m = torch.zeros(x.numel(), dtype=torch.bool)
    m[::7] = True
    return torch.where(m.view(x.shape), t, x)


CASES = [((4, 16, 14, 14), False), ((64, 3, 7, 7), True), ((1000, 512), True), ((7, 13, 3), True), ((5, 4099), True),
         ((1,), False), ((1, 5), True), ((3, 1, 1), True), ((33,), False), ((2, 70001), False), ((3000, 1), True)]


def _case(shape, per_channel, sym, n_bits, nonneg, pt_delta=None):
    """(quantizer with CPU-chain range buffers, its degenerate channels planted; x with ties and NaNs; number of NaNs)"""
    g = torch.Generator().manual_seed(hash((shape, n_bits)) % 1000)
    x = _adversarial(shape, g)
    C = shape[0] if per_channel else 1
    xmin = (-torch.rand(C, generator=g) * 4) if per_channel else -torch.rand((), generator=g) * 4
    xmax = (torch.rand(C, generator=g) * 4) if per_channel else torch.rand((), generator=g) * 4
    if per_channel and C > 2:
        xmin[1] = 0.0
        xmax[1] = 0.0                                # degenerate channel: xmin == xmax == 0
        xmin[2] = 0.25                               # positive minimum
    if nonneg:
        xmin = xmin.abs()                            # non-negative ranges (symmetric: unsigned)
    qc = _quantizer(sym, n_bits, per_channel)
    qc.set_quant_range(xmin, xmax)                   # the eager chain on the CPU
    x = _ties(x, qc)
    # degenerate scales, from the end of the channel list: NaN, inf, 0
    d = qc._delta.clone()
    if per_channel:
        for back, v in ((1, float("nan")), (2, float("inf")), (3, 0.0)):
            if C >= back + 3:
                d[C - back] = v
    elif pt_delta is not None:
        d.fill_(pt_delta)
    qc._delta = d
    f = x.reshape(-1)
    nan_at = torch.arange(5, max(f.numel(), 5), 13)
    f[nan_at] = float("nan")
    return qc, f.view(shape), int(nan_at.numel())


def _code_of_float(t, n_bits):
    """a float tensor of integers as raw storage codes"""
    if n_bits <= 8:
        return (t.to(torch.int32) & 255).to(torch.uint8)
    return (t.to(torch.int32) & 65535).to(torch.int32).to(torch.int16)     # wraps: the raw two's-complement bits


def _check_case(qc, x, n_nan, n_bits, sym):
    from fp8q import ops
    q = _with_buffers(qc, "cuda")
    qb = _with_buffers(qc, "cuda")
    xg = x.cuda()
    args = (q._delta, None if sym else q._zero_float, q._signed if sym else None, n_bits, sym, q.eps)
    n = x.numel()
    wide = n_bits > 8
    cdt = torch.int16 if wide else torch.uint8

    # (1) to_integer == the eager CUDA chain on copies of the same buffers
    with _Eager():
        t_ref = qb.to_integer_forward(xg)
    t = ops.int_to_integer(xg, *args)
    assert _same_nan(t, t_ref)
    assert _same_nan(q.to_integer_forward(xg), t_ref)

    # (2) encode == (1) cast to the storage type; NaN -> the code of zp (0 when symmetric)
    codes = ops.int_encode(xg, *args)
    assert codes.dtype == cdt and codes.shape == x.shape and codes.is_contiguous()
    zp = torch.zeros_like(t_ref) if sym else qb._params_like(xg)[1].expand_as(t_ref)
    want = torch.where(t_ref.isnan(), zp.nan_to_num(0.0), t_ref)
    assert torch.equal(codes.cpu(), _code_of_float(want.cpu(), n_bits))
    signed = sym and bool(qc._signed)
    ints = (codes.view(torch.int8) if not wide else codes).int() if signed else \
        (codes.int() & 65535 if wide else codes.int())
    assert int(ints.min()) >= (-(2 ** (n_bits - 1)) if signed else 0)
    assert int(ints.max()) <= (2 ** (n_bits - 1) - 1 if signed else 2 ** n_bits - 1)

    # (3) decode(encode(x)) == int_quantize(x), every element whose x is not NaN
    y = ops.int_quantize(xg, *args)
    yd = ops.int_decode(codes, *args)
    keep = ~xg.isnan()
    compared = int(keep.sum())
    assert compared >= n - n_nan
    assert torch.equal(yd.view(torch.int32)[keep], y.view(torch.int32)[keep])

    # views that are not co-aligned: x one element off a 16-byte boundary, codes / out one element (1 byte, 2 bytes, 4
    # bytes) off theirs -- the element-wise paths -- against the aligned results above
    xo = torch.empty(n + 1, device="cuda")[1:].view(x.shape).copy_(xg)
    assert xo.data_ptr() % 16 == 4
    assert torch.equal(ops.int_encode(xo, *args), codes)
    assert _same_nan(ops.int_to_integer(xo, *args), t)
    co = torch.empty(n + 1, dtype=cdt, device="cuda")[1:].view(x.shape)
    assert co.data_ptr() % 16 == (2 if wide else 1)
    assert ops.int_encode(xg, *args, out=co) is co and torch.equal(co, codes)
    assert _same_nan(ops.int_decode(co, *args), yd)
    yo = torch.empty(n + 1, device="cuda")[1:].view(x.shape)
    assert _same_nan(ops.int_decode(codes, *args, out=yo), yd)
    assert _same_nan(ops.int_to_integer(xg, *args, out=yo), t)


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("n_bits", [2, 4, 8, 9, 16])
@pytest.mark.parametrize("shape,per_channel", CASES)
def test_codes_equal_the_eager_chain_and_round_trip(sym, n_bits, shape, per_channel):
    for nonneg in (False, True):
        qc, x, n_nan = _case(shape, per_channel, sym, n_bits, nonneg)
        _check_case(qc, x, n_nan, n_bits, sym)


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("n_bits", [8, 16])
@pytest.mark.parametrize("delta", [0.0, float("inf"), float("nan")])
def test_degenerate_per_tensor_scale(sym, n_bits, delta):
    qc, x, n_nan = _case((3, 1500), False, sym, n_bits, False, pt_delta=delta)
    _check_case(qc, x, n_nan, n_bits, sym)


GU_CASES = [(q, pc, nb) for q in ("sym", "asym") for pc in (0, 1) for nb in (2, 4, 8, 16)]


@pytest.fixture(scope="module")
def gu():
    return np.load(os.path.join(HERE, "golden", "gu1_uniform.npz")), np.load(os.path.join(HERE, "golden", "gu2_uniform_int.npz"))


@pytest.mark.parametrize("qname,pc,nb", GU_CASES)
def test_to_integer_equals_the_reference(gu, qname, pc, nb):
    from fp8q import ops
    g1, g2 = gu
    case = f"{qname}_pc{pc}_b{nb}"
    rec = case + "_current_minmax"
    sym = qname == "sym"
    for i, x in enumerate(g1[case + "_x"]):
        d = torch.from_numpy(g1[rec + "_delta"][i].copy()).cuda()
        zf = None if sym else torch.from_numpy(g1[rec + "_zf"][i].copy()).cuda()
        sg = torch.tensor([bool(g1[rec + "_signed"][i])], device="cuda") if sym else None
        t = ops.int_to_integer(torch.from_numpy(x).cuda(), d, zf, sg, nb, sym, 1e-8)
        assert _same_nan(t, torch.from_numpy(g2[case + "_t"][i])), (case, i)


def _fixed(sym, per_channel, n_bits=8):
    q = _quantizer(sym, n_bits, per_channel)
    if per_channel:
        q.set_quant_range(torch.full((4,), -1.0, device="cuda"), torch.full((4,), 2.0, device="cuda"))
        return q, torch.randn(4, 9, device="cuda")
    q.set_quant_range(torch.tensor(-1.0, device="cuda"), torch.tensor(2.0, device="cuda"))
    return q, torch.randn(100, device="cuda")


def test_the_kernel_path_is_taken(monkeypatch):
    from fp8q import Fp8qError
    qs, xs = _fixed(True, False)
    qa, xa = _fixed(False, True)

    def boom(*a, **k):
        raise AssertionError("eager chain used")
    monkeypatch.setattr(torch, "round", boom)
    for q, x in ((qs, xs), (qa, xa)):
        t = q.to_integer_forward(x)
        c = q.encode(x)
        y = q.decode(c)
        assert t.dtype == torch.float32 and c.dtype == torch.uint8 and _same(y, q(x))
    monkeypatch.setenv("FP8Q_INT_KERNELS", "0")
    for q, x in ((qs, xs), (qa, xa)):
        with pytest.raises(AssertionError, match="eager chain"):
            q.to_integer_forward(x)
        with pytest.raises(Fp8qError):
            q.encode(x)
        with pytest.raises(Fp8qError):
            q.decode(c)


def test_encode_and_decode_raise_off_the_kernel_path():
    from fp8q import Fp8qError, ops
    q, x = _fixed(False, True)
    with pytest.raises(Fp8qError):
        q.encode(x.cpu())
    with pytest.raises(Fp8qError):
        q.encode(x.double())
    with pytest.raises(Fp8qError):
        q.decode(q.encode(x).cpu())
    with pytest.raises(Fp8qError):
        q.decode(x)                                          # float "codes"
    with pytest.raises(Fp8qError):
        ops.int_encode(x.cpu(), q._delta, q._zero_float)
    with pytest.raises(Fp8qError):
        ops.int_decode(q.encode(x).view(torch.int8), q._delta, q._zero_float)
    with pytest.raises(Fp8qError):
        ops.int_encode(x, q._delta, q._zero_float, out=torch.empty(4, 9, dtype=torch.int16, device="cuda"))


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("per_channel", [False, True])
def test_no_host_synchronisation(sym, per_channel):
    q, x = _fixed(sym, per_channel)
    q.decode(q.encode(x))                                    # load the library, warm the allocator
    q.to_integer_forward(x)
    with _NoSync():
        t = q.to_integer_forward(x)
        c = q.encode(x)
        y = q.decode(c)
    assert _same(y, q(x)) and torch.equal(c.cpu(), _code_of_float(t.cpu(), 8))


@pytest.mark.parametrize("sym", [True, False])
def test_to_integer_forward_stays_differentiable(sym):
    q, x = _fixed(sym, False)
    x.requires_grad_(True)
    t = q.to_integer_forward(x)
    assert t.requires_grad
    t.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and bool((x.grad != 0).any())


def test_the_symmetric_sign_is_read_on_the_device():
    q, _ = _fixed(True, False)
    assert bool(q._signed)
    x = -torch.rand(5000, device="cuda") - 0.01              # negative data
    q.encode(x)
    with _NoSync():
        a = q.encode(x)
        q._signed.fill_(False)                               # in place: nothing on the host learns of it
        b = q.encode(x)
    assert int(a.view(torch.int8).max()) < 0 and int(a.view(torch.int8).min()) >= -128     # two's-complement negatives
    assert int(b.max()) == 0                                 # unsigned: clamped to int_min == 0
    with _NoSync():
        ya = q.decode(b)
    assert bool((ya == 0).all())
