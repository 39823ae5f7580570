"""Storage codes of the half-precision lane on the GPU (csrc/fp8q_codec_h16.hip): encoding an fp16 / bf16 tensor gives, byte
for byte, the codes of the exactly widened tensor -- the oracle's for FP8, the float32 kernel's for INT (itself pinned to the
reference by test_int_codes_golden.py) -- and decoding to a half type gives the float32 value rounded once by torch.
Equality means equal bit patterns, except that a NaN matches any NaN."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
FORMATS = ((8, 2, 1), (8, 3, 1), (8, 4, 1), (8, 3, 0), (6, 2, 1))       # (n_bits, M, sign_bits)
MAXVALS = (0.37, 1.0, 448.0, 3e-5, 6e4)
GUARD = 64


def _ops():
    from fp8q import ops
    return ops


class _NoSync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


def _same_nan(a, b):
    """a, b tensors of one dtype on one device: NaN at the same places, equal bits elsewhere"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    same = torch.equal(a.isnan(), b.isnan())
    return same and torch.equal(a.nan_to_num(0.0).contiguous().view(it), b.nan_to_num(0.0).contiguous().view(it))


def _all_patterns(dtype):
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def _int_ranges(n_bits, sym, n=1, dev="cuda"):
    """(delta, zero_float, signed_flag) of n channels: a grid that clips part of the inputs, a nonzero zero point"""
    delta = torch.full((n,), 7.5 / 2 ** n_bits, device=dev)
    if sym:
        return delta, None, torch.ones(1, dtype=torch.uint8, device=dev)
    return delta, torch.full((n,), 0.3 * (2 ** n_bits - 1) + 0.4, device=dev), None


# ---- 1. exhaustive inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_encode_every_input(dtype):
    ops = _ops()
    x = _all_patterns(dtype)
    xf, xd = x.float().numpy(), x.cuda()
    bad = []
    for n_bits, M, s in FORMATS:
        for mval in MAXVALS:
            mv = np.array([mval], np.float32)
            want = oracle.c_encode(xf, mv, float(M), n_bits, s)
            got = ops.encode(xd, torch.from_numpy(mv).cuda(), float(M), n_bits, s)
            assert got.dtype == torch.uint8 and got.shape == x.shape
            diff = int((got.cpu().numpy() != want).sum())
            if diff:
                bad.append((n_bits, M, s, mval, diff))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
def test_int_encode_every_input(dtype):
    ops = _ops()
    xd = _all_patterns(dtype).cuda()
    xf = xd.float()
    bad = []
    for n_bits in (2, 4, 8, 9, 16):
        for sym in (True, False):
            d, z, sg = _int_ranges(n_bits, sym)
            cases = [("grid", d, z, sg)]
            if sym:
                cases.append(("unsigned", d, z, torch.zeros(1, dtype=torch.uint8, device="cuda")))
            for degenerate in (0.0, float("inf"), float("nan")):
                cases.append((str(degenerate), torch.full((1,), degenerate, device="cuda"), z, sg))
            for name, dd, zz, ss in cases:
                want = ops.int_encode(xf, dd, zz, ss, n_bits, sym)
                got = ops.int_encode(xd, dd, zz, ss, n_bits, sym)
                assert got.dtype == want.dtype == (torch.uint8 if n_bits <= 8 else torch.int16)
                if not torch.equal(got, want):
                    bad.append((n_bits, sym, name, int((got != want).sum())))
    assert not bad, bad


# ---- 2. exhaustive codes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_decode_every_code(dtype):
    ops = _ops()
    bad = []
    overflow = False
    for n_bits, M, s in FORMATS:
        codes = np.arange(2 ** n_bits, dtype=np.uint8)
        for mval in MAXVALS + (3e5,):                                   # 3e5: beyond float16's largest finite value
            mv = np.array([mval], np.float32)
            want = torch.from_numpy(oracle.c_decode(codes, mv, float(M), n_bits, s)).to(dtype)
            got = ops.decode(torch.from_numpy(codes).cuda(), torch.from_numpy(mv).cuda(), float(M), n_bits, s, out_dtype=dtype)
            assert got.dtype == dtype
            overflow |= bool(want.isinf().any())
            if not _same_nan(got.cpu(), want):
                bad.append((n_bits, M, s, mval))
    assert not bad, bad
    assert overflow == (dtype == torch.float16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_int_decode_every_code(dtype):
    ops = _ops()
    bad = []
    overflow = False
    for n_bits, codes in ((8, torch.arange(256, dtype=torch.int32).to(torch.uint8)),
                          (16, torch.arange(65536, dtype=torch.int32).to(torch.int16)),
                          (5, torch.arange(256, dtype=torch.int32).to(torch.uint8)),
                          (12, torch.arange(65536, dtype=torch.int32).to(torch.int16))):
        codes = codes.cuda()
        delta = torch.tensor([1000.0 if n_bits <= 8 else 7.0], device="cuda")       # 255 * 1000, 65535 * 7 > 65504
        cases = [(True, None, torch.ones(1, dtype=torch.uint8, device="cuda")),     # read as signed
                 (True, None, torch.zeros(1, dtype=torch.uint8, device="cuda")),    # ... and as unsigned
                 (False, torch.tensor([0.3 * 2 ** n_bits + 0.4], device="cuda"), None)]
        for sym, z, sg in cases:
            want = ops.int_decode(codes, delta, z, sg, n_bits, sym).to(dtype)
            got = ops.int_decode(codes, delta, z, sg, n_bits, sym, out_dtype=dtype)
            assert got.dtype == dtype
            overflow |= bool(want.isinf().any())
            if not _same_nan(got, want):
                bad.append((n_bits, sym, None if sg is None else int(sg)))
    assert not bad, bad
    assert overflow == (dtype == torch.float16)


# ---- 3. shapes and alignment ---------------------------------------------------------------------------------------------
SHAPES = [(C, inner) for inner in (1, 3, 7, 8, 9, 15, 147, 1023, 4097, 65536 + 5) for C in (1, 5, 64, 1000)
          if C * inner <= 1 << 24]


SHORT_ROW_FORMATS = {8: ((8, 5, 1), (6, 3, 1)), 9: ((8, 4, 1), (6, 2, 1)), 15: ((6, 2, 1), (8, 4, 1))}


def _planted(C, inner, dtype, row_scale, seed):
    """[C, inner] on the GPU: row c drawn at the scale of its own range; NaN, +-inf and -0 planted"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(C, inner, generator=g, device="cuda") * torch.exp(0.5 * torch.randn(C, inner, generator=g, device="cuda"))
    x = (x * row_scale[:, None]).to(dtype).reshape(-1)
    n = x.numel()
    for k, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0)):
        for pos in (k, n // 2 + k, n - 1 - k):
            if 0 <= pos < n:
                x[pos] = v
    return x.view(C, inner)


def _window(n, dtype, phase, fill):
    """(whole buffer, an n-element window `phase` elements behind GUARD sentinels)"""
    buf = torch.full((n + 2 * GUARD + 1,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD + phase:GUARD + phase + n]


def _guards(buf, n, phase, fill):
    return (buf[:GUARD + phase] == fill).all() & (buf[GUARD + phase + n:] == fill).all()


def _eq(a, b):
    """0-dim bool tensor (no host round trip): equal bits, a NaN matching any NaN"""
    if a.is_floating_point():
        it = {4: torch.int32, 2: torch.int16}[a.element_size()]
        return ((a.isnan() == b.isnan()).all()
                & (a.nan_to_num(0.0).contiguous().view(it) == b.nan_to_num(0.0).contiguous().view(it)).all())
    return (a == b).all()


@pytest.mark.parametrize("family", ["fp8", "int8", "int16"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_and_alignment(dtype, family):
    """per channel and per tensor on [C, inner]; x contiguous and as the view base[1:] (a 2-byte phase); the codes written at
    element phases 0 and 1 of guarded buffers, decoded from those views into guarded half buffers at both phases.  The
    ranges of neighbouring rows lie six orders of magnitude and more apart: a group that took the wrong row's table would
    give other codes.  Yardstick: the float32 kernels on the widened tensor, their values rounded by torch."""
    ops = _ops()
    code_dt = torch.int16 if family == "int16" else torch.uint8
    fill_c = 0x5A
    bad = []
    for k, (C, inner) in enumerate(SHAPES):
        rows = torch.arange(C, device="cuda")
        scale = torch.where(rows % 2 == 0, 2e-3, 3e3) * (1.0 + 0.01 * (rows % 7))       # neighbours: ~1.5e6 apart
        x = _planted(C, inner, dtype, scale, 1000 + k)
        xf = x.float()
        n = C * inner
        base = torch.zeros(n + 1, dtype=dtype, device="cuda")
        base[1:] = x.reshape(-1)
        views = (("contig", x), ("view", base[1:].view(C, inner)))
        assert views[1][1].data_ptr() % 4 == 2
        if family == "fp8":
            # rows of 8 .. 15 elements reach the chunk kernels (the straddling paths) only while the tables of a 4096-element
            # chunk fit 40 KiB of LDS: two exponent bits for rows of 8, three from 9 on; other formats go thread = row there
            n_bits, M, s = SHORT_ROW_FORMATS[inner][k % 2] if inner in SHORT_ROW_FORMATS else FORMATS[k % len(FORMATS)]
            per_row = (scale * 2.0,)
            fixed = (float(M), n_bits, s)
            enc, dec = ops.encode, ops.decode
        else:
            n_bits, sym = (8 if family == "int8" else (16, 11)[k % 2]), bool((k // 2) % 2)
            delta = scale * 6.0 / 2 ** n_bits
            zf = None if sym else (0.3 + 0.05 * (rows % 5)) * (2 ** n_bits - 1) + 0.4
            sg = torch.ones(1, dtype=torch.uint8, device="cuda") if sym else None
            per_row = (delta, zf, sg)
            fixed = (n_bits, sym)
            enc, dec = ops.int_encode, ops.int_decode
        for pc in (True, False):
            if family == "fp8":
                rng = per_row if pc else (per_row[0].amax().reshape(1),)
            else:
                rng = per_row if pc else (per_row[0][-1:].clone(), None if per_row[1] is None else per_row[1][-1:].clone(),
                                          per_row[2])
            want_c = enc(xf, *rng, *fixed)
            want_y = dec(want_c, *rng, *fixed).to(dtype)
            ok = torch.ones((), dtype=torch.bool, device="cuda")
            for vname, xd in views:
                for cph in (0, 1):
                    cbuf, cwin = _window(n, code_dt, cph, fill_c)
                    got = enc(xd, *rng, *fixed, out=cwin)
                    assert got.data_ptr() == cwin.data_ptr() and cwin.data_ptr() // cwin.element_size() % 2 == cph
                    ok &= _eq(cwin.view(C, inner), want_c) & _guards(cbuf, n, cph, fill_c)
                    if vname == "view":
                        continue                                         # (decoding does not depend on where x lay)
                    for yph in (0, 1):
                        ybuf, ywin = _window(n, dtype, yph, 7.0)
                        dec(cwin.view(C, inner), *rng, *fixed, out=ywin)
                        assert ywin.data_ptr() // 2 % 2 == yph
                        ok &= _eq(ywin.view(C, inner), want_y) & _guards(ybuf, n, yph, 7.0)
            if not bool(ok):
                bad.append((C, inner, pc, fixed))
    assert not bad, bad


# ---- 4. round trips ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trips_equal_the_quantizers(dtype):
    ops = _ops()
    bad = []
    for k, (C, inner) in enumerate(((64, 147), (5, 4097), (1000, 9), (3, 65541))):
        rows = torch.arange(C, device="cuda")
        scale = 10.0 ** ((rows % 7).float() - 3.0)                       # maxval within [1e-3, 1e3]
        x = _planted(C, inner, dtype, scale, 50 + k)
        finite = torch.where(x.isnan(), torch.zeros_like(x), x)          # (the FP8 codes have no NaN)
        for n_bits, M, s in FORMATS:
            for mv in (scale, scale.amax().reshape(1)):
                got = ops.decode(ops.encode(finite, mv, float(M), n_bits, s), mv, float(M), n_bits, s, out_dtype=dtype)
                want = ops.quantize(finite, mv, float(M), n_bits, s, out_dtype=dtype)
                if not _same_nan(got, want):
                    bad.append(("fp8", C, inner, n_bits, M, s, mv.numel()))
        notnan = ~x.isnan()
        for n_bits in (4, 8, 16):
            for sym in (True, False):
                d, z, sg = _int_ranges(n_bits, sym, C)
                d = d * scale
                for rng in ((d, z, sg), (d[-1:].clone(), None if z is None else z[-1:].clone(), sg)):
                    got = ops.int_decode(ops.int_encode(x, *rng, n_bits, sym), *rng, n_bits, sym, out_dtype=dtype)
                    want = ops.int_quantize(x, *rng, n_bits, sym, out_dtype=dtype)
                    if not _same_nan(got[notnan], want[notnan]):
                        bad.append(("int", C, inner, n_bits, sym, rng[0].numel()))
    assert not bad, bad


# ---- 5. size-selected variants -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_large_tensors_take_the_wide_chunks(dtype, pc):
    """from 2^19 groups of 16 elements on, the FP8 kernels run 8192-element chunks with two groups per lane (U = 2): one
    tensor beyond that, x at an odd start, against the float32 entry points on x.float().  The INT kernels have one geometry."""
    ops = _ops()
    C, inner = 228263, 147                                               # 33.5 M elements
    n = C * inner
    g = torch.Generator(device="cuda").manual_seed(3)
    base = torch.randn(n + 1, generator=g, device="cuda").to(dtype)
    for k, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0)):
        for pos in (1 + k, n // 2 + k, n - k):
            base[pos] = v
    xd = base[1:].view(C, inner)
    assert xd.data_ptr() % 4 == 2
    xf = xd.float()
    n_bits, M, s = (8, 2, 1) if pc else (8, 3, 1)
    mv = xf.nan_to_num(0.0, 0.0, 0.0).abs().amax(1) * 0.9 if pc else torch.tensor([2.5], device="cuda")
    want_c = ops.encode(xf, mv, float(M), n_bits, s)
    want_y = ops.decode(want_c, mv, float(M), n_bits, s).to(dtype)
    del xf
    cph = 1 if pc else 0                                                 # byte stores / one 16-byte store per lane
    cbuf, cwin = _window(n, torch.uint8, cph, 0x5A)
    ops.encode(xd, mv, float(M), n_bits, s, out=cwin)
    assert bool(_eq(cwin.view(C, inner), want_c) & _guards(cbuf, n, cph, 0x5A))
    ybuf, ywin = _window(n, dtype, 1, 7.0)
    ops.decode(cwin.view(C, inner), mv, float(M), n_bits, s, out=ywin)
    assert bool(_eq(ywin.view(C, inner), want_y) & _guards(ybuf, n, 1, 7.0))


# ---- 6. no host synchronisation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_four_ops_only_enqueue(dtype):
    ops = _ops()
    C, inner = 64, 147
    x = torch.randn(C, inner, device="cuda").to(dtype)
    mv = x.float().abs().amax(1)
    d, z, sg = _int_ranges(8, False, C)
    d16, _, sg16 = _int_ranges(16, True, C)
    c8 = torch.empty(C, inner, dtype=torch.uint8, device="cuda")
    c16 = torch.empty(C, inner, dtype=torch.int16, device="cuda")
    y = torch.empty(C, inner, dtype=dtype, device="cuda")
    ops.encode(x, mv, 3.0, out=c8)                                       # (the library is loaded before the guarded block)
    with _NoSync():
        ops.encode(x, mv, 3.0, out=c8)
        ops.decode(c8, mv, 3.0, out=y)
        ops.decode(c8, mv, 3.0, out_dtype=dtype)
        ops.int_encode(x, d, z, None, 8, False, out=c8)
        ops.int_decode(c8, d, z, None, 8, False, out=y)
        ops.int_encode(x, d16, None, sg16, 16, True, out=c16)
        ops.int_decode(c16, d16, None, sg16, 16, True, out_dtype=dtype)
    torch.cuda.synchronize()
