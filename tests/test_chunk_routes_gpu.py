"""The chunked kernels (csrc/fp8q_intq.h's geometry: k_int_quant, k_inth16_quant, k_int_level / k_int_encode / k_int_decode and
their half forms, k_ocp) at every rows-per-chunk case of tests/chunk_cases.py, bit for bit against the oracle each lane's own
test uses: the quantizer classes on CPU tensors for the INT lanes (ranges from the CPU chain too), torch's CPU cast for the
hardware FP8 lane (tests/test_ocp_gpu.py).  NaNs are compared by position.  Every case asserts ops.chunk_route first, so a
changed threshold fails loudly and no branch silently loses its test.  tests/test_chunk_routes_host.py shows that these inputs
would see a wrong row index, a short LDS table or a partial sign fold."""
import numpy as np
import pytest
import torch

import chunk_cases as cc

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
KEYS = list(cc.SHAPES)
INT_CASES = [(k, 8) for k in KEYS] + [(k, b) for k in cc.WIDE_BITS for b in (2, 16)]
FMT = {"e4m3fn": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def _id(v):
    if isinstance(v, tuple):
        return "x".join(str(int(i)) if not isinstance(i, bool) else ("pc" if i else "pt") for i in v)
    return str(v).replace("torch.", "")


def _same(got, want, what):
    """equal bit patterns, NaN meeting NaN at the same place"""
    g, w = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if g.is_floating_point():
        assert torch.equal(g.isnan(), w.isnan()), f"{what}: NaNs at other places"
        it = torch.int32 if g.dtype == torch.float32 else torch.int16
        g, w = g.nan_to_num(0.0).view(it), w.nan_to_num(0.0).view(it)
    bad = (g != w).flatten().nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {g.numel()} differ, first at {bad[:5].tolist()}: " \
                             f"{g.flatten()[bad[:5]].tolist()} != {w.flatten()[bad[:5]].tolist()}"


def _codes_of(t, n_bits):
    """a float tensor of integers as raw storage codes"""
    if n_bits <= 8:
        return (t.to(torch.int32) & 255).to(torch.uint8)
    return (t.to(torch.int32) & 65535).to(torch.int16)


def _quantizer(sym, n_bits, pc, xmin, xmax):
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    q = (SymmetricUniformQuantizer if sym else AsymmetricUniformQuantizer)(n_bits=n_bits, per_channel=pc)
    q.set_quant_range(torch.from_numpy(xmin), torch.from_numpy(xmax))      # the eager chain on the CPU
    return q


_cache = {}


def _int_ref(key, n_bits, sym, dtype=torch.float32):
    """the case and its CPU-chain results, computed once and never modified: x (as dtype), y, t, codes, decoded"""
    ck = (key, n_bits, sym, dtype)
    if ck not in _cache:
        case = cc.int_case(key, n_bits, sym)
        q = _quantizer(sym, n_bits, key[2], case["xmin"], case["xmax"])
        x = torch.from_numpy(case["x"]).to(dtype)
        xf = x.float()
        x0 = torch.where(xf.isnan(), torch.zeros_like(xf), xf)            # a NaN has no code: it stores the code of the value 0
        _cache[ck] = dict(case=case, q=q, x=x, y=q(xf), t=q.to_integer_forward(xf) + 0.0,      # (a zero level is +0)
                          codes=_codes_of(q.to_integer_forward(x0), n_bits), dec=q(x0))
    return _cache[ck]


def _range_args(q, sym):
    return (q._delta.cuda(), None if sym else q._zero_float.cuda(), q._signed.cuda() if sym else None)


def _sentinel(n, dtype=torch.float32):
    if dtype == torch.uint8:
        return torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(buf, C):
    t = buf[C:]
    return bool((t == 0x5A).all()) if buf.dtype == torch.uint8 else bool((t.view(torch.int32) == SENTINEL).all())


def _check_route(ops, key, want_vec=True, **kw):
    r = cc.route_of(ops, key, **kw)
    want = dict(cc.SHAPES[key], vec=want_vec and kw.get("elem_bytes", 4) == 4)
    want["sign_prepass"] = bool(kw.get("symmetric") and kw.get("sets_range") and key[0] > cc.SIGN_INLINE and key[2])
    assert all(r[k] == v for k, v in want.items()), (key, kw, r, want)
    return r


def _range_launch(ops, key, n_bits, sym, x, xmin, xmax, q, y_ref, out_dtype=None, what=""):
    """a range-setting launch into sentinel-filled buffers 64 entries longer than the range: every entry below C equals the CPU
    chain, every entry from C up still holds the sentinel"""
    C = xmin.numel()
    dbuf, zbuf, sbuf = _sentinel(C + 64), _sentinel(C + 64), _sentinel(1 + 64, torch.uint8)
    y, d, z, sg = ops.int_range_quantize(x, xmin, xmax, n_bits, sym, delta=dbuf[:C], zero_float=None if sym else zbuf[:C],
                                         signed_flag=sbuf[:1] if sym else None, out_dtype=out_dtype)
    _same(y, y_ref, what + " range_quantize")
    _same(dbuf[:C], q._delta.reshape(-1), what + " delta")
    assert _untouched(dbuf, C), what + ": delta written past C - 1"
    if sym:
        assert int(sbuf[0]) == int(bool(q._signed)) and _untouched(sbuf, 1), what + " sign"
        assert _untouched(zbuf, 0)
    else:
        _same(zbuf[:C], q._zero_float.reshape(-1), what + " zero_float")
        assert _untouched(zbuf, C) and _untouched(sbuf, 0), what + ": zero_float written past C - 1"


@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("key,n_bits", INT_CASES, ids=_id)
def test_int_fp32(key, n_bits, sym):
    """int_quantize, int_range_quantize, int_to_integer, int_encode, int_decode on float32"""
    from fp8q import ops
    ref = _int_ref(key, n_bits, sym)
    q, what = ref["q"], f"{key} {n_bits} {'sym' if sym else 'asym'}"
    xg = ref["x"].cuda()
    assert xg.data_ptr() % 16 == 0
    _check_route(ops, key, symmetric=sym)
    args = _range_args(q, sym) + (n_bits, sym, q.eps)
    _same(ops.int_quantize(xg, *args), ref["y"], what + " quantize")
    _same(ops.int_to_integer(xg, *args), ref["t"], what + " to_integer")
    codes = ops.int_encode(xg, *args)
    _same(codes, ref["codes"], what + " encode")
    _same(ops.int_decode(codes, *args), ref["dec"], what + " decode")
    _check_route(ops, key, symmetric=sym, sets_range=True)
    xmin, xmax = torch.from_numpy(ref["case"]["xmin"]).cuda(), torch.from_numpy(ref["case"]["xmax"]).cuda()
    _range_launch(ops, key, n_bits, sym, xg, xmin, xmax, q, ref["y"], what=what)


@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=_id)
@pytest.mark.parametrize("key", KEYS, ids=_id)
def test_int_half(key, dtype, sym):
    """the same on float16 / bfloat16 tensors (csrc/fp8q_inth16.hip, the INT part of csrc/fp8q_codec_h16.hip): the CPU chain on
    the exactly widened tensor, one rounding back"""
    from fp8q import ops
    ref = _int_ref(key, 8, sym, dtype)
    q, what = ref["q"], f"{key} {dtype} {'sym' if sym else 'asym'}"
    xg = ref["x"].cuda()
    assert xg.data_ptr() % 16 == 0
    _check_route(ops, key, elem_bytes=2, symmetric=sym)
    args = _range_args(q, sym) + (8, sym, q.eps)
    _same(ops.int_quantize(xg, *args), ref["y"], what + " quantize -> f32")
    _same(ops.int_quantize(xg, *args, out_dtype=dtype), ref["y"].to(dtype), what + " quantize -> half")
    codes = ops.int_encode(xg, *args)
    _same(codes, ref["codes"], what + " encode")
    _same(ops.int_decode(codes, *args, out_dtype=dtype), ref["dec"].to(dtype), what + " decode -> half")
    _check_route(ops, key, elem_bytes=2, symmetric=sym, sets_range=True)
    xmin, xmax = torch.from_numpy(ref["case"]["xmin"]).cuda(), torch.from_numpy(ref["case"]["xmax"]).cuda()
    _range_launch(ops, key, 8, sym, xg, xmin, xmax, q, ref["y"], out_dtype=torch.float32, what=what + " -> f32")
    _range_launch(ops, key, 8, sym, xg, xmin, xmax, q, ref["y"].to(dtype), out_dtype=dtype, what=what + " -> half")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_id)
@pytest.mark.parametrize("fmt", ["e4m3fn", "e5m2"])
@pytest.mark.parametrize("key", KEYS, ids=_id)
def test_ocp(key, fmt, dtype):
    """encode (codes and scale_out), decode and quantize of the hardware FP8 lane, by tests/test_ocp_gpu.py's own check"""
    from fp8q import ops
    from fp8q._lib import lib
    from test_ocp_gpu import _check_lane, _oracle
    C, inner, pc = key
    case = cc.ocp_case(key, fmt)
    x, maxval = torch.from_numpy(case["x"]).to(dtype), torch.from_numpy(case["maxval"])
    _check_route(ops, key)
    _check_lane(x, maxval, FMT[fmt], pc, f"{key} {fmt} {dtype}")
    if dtype == torch.float32:
        # scale_out into a sentinel-filled buffer 64 entries longer than the range
        n = maxval.numel()
        xg, mg = x.cuda(), maxval.cuda()
        codes, sbuf = torch.empty(x.shape, dtype=torch.uint8, device="cuda"), _sentinel(n + 64)
        rc = lib().fp8q_ocp_encode_f32(xg.data_ptr(), codes.data_ptr(), C if pc else 1, inner if pc else C * inner,
                                       mg.data_ptr(), n, 0 if fmt == "e4m3fn" else 1, 1e-8, sbuf.data_ptr(),
                                       ops._stream(xg))
        assert rc == 0
        ref_c, ref_s, _ = _oracle(x, maxval, FMT[fmt], pc)
        _same(sbuf[:n], ref_s, "scale_out")
        assert _untouched(sbuf, n), "scale_out written past C - 1"
        _same(codes, ref_c.view(torch.uint8), "codes")


@pytest.mark.parametrize("name", ["last_negative", "negative_at_1500", "nan_last", "non_negative"])
@pytest.mark.parametrize("C", cc.SIGN_C)
def test_the_sign_fold_reads_the_whole_vector(C, name):
    """C = 2048: every block folds x_min itself with 256 threads; C = 2049: k_int_sign with 1024.  The sign and the quantized
    tensor, through int_range_quantize and through int_set_range."""
    from fp8q import ops
    case = cc.sign_case(C, name)
    q = _quantizer(True, 8, True, case["xmin"], case["xmax"])
    assert bool(q._signed) == case["sign"]
    x = torch.from_numpy(case["x"])
    y_ref = q(x)
    r = ops.chunk_route(C, 2, symmetric=True, sets_range=True)
    assert r["sign_prepass"] == (C > cc.SIGN_INLINE) and r["rows_per_chunk"] == C
    xmin, xmax = torch.from_numpy(case["xmin"]).cuda(), torch.from_numpy(case["xmax"]).cuda()
    _range_launch(ops, (C, 2, True), 8, True, x.cuda(), xmin, xmax, q, y_ref, what=f"{C} {name}")
    for start in (0x5A, 0, 1):                  # whatever the byte held before
        sbuf = torch.full((65,), start, dtype=torch.uint8, device="cuda")
        d, _, sg = ops.int_set_range(xmin, xmax, 8, True, signed_flag=sbuf[:1])
        assert int(sbuf[0]) == int(case["sign"]) and bool((sbuf[1:] == start).all()), (C, name, start)
        _same(d, q._delta, f"{C} {name} set_range delta")
        _same(ops.int_quantize(x.cuda(), d, None, sg, 8, True), y_ref, f"{C} {name} quantize after set_range")


def _off(t, elems=1):
    """a copy of t that starts `elems` elements behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == elems * t.element_size()
    return v


@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("key", cc.UNALIGNED, ids=_id)
def test_unaligned_int(key, sym):
    """the input, the output, and both one element off a 16-byte boundary -- the element-by-element instances -- against the
    aligned call, which test_int_fp32 holds against the oracle"""
    from fp8q import ops
    ref = _int_ref(key, 8, sym)
    q = ref["q"]
    xg = ref["x"].cuda()
    args = _range_args(q, sym) + (8, sym, q.eps)
    xmin, xmax = torch.from_numpy(ref["case"]["xmin"]).cuda(), torch.from_numpy(ref["case"]["xmax"]).cuda()
    ya, ta, ca = ops.int_quantize(xg, *args), ops.int_to_integer(xg, *args), ops.int_encode(xg, *args)
    da = ops.int_decode(ca, *args)
    ra = ops.int_range_quantize(xg, xmin, xmax, 8, sym)[0]
    for off_in, off_out in ((True, False), (False, True), (True, True)):
        what = f"{key} in{'+1' if off_in else ''} out{'+1' if off_out else ''}"
        xi, ci = (_off(xg) if off_in else xg), (_off(ca) if off_in else ca)
        fo = (lambda: _off(torch.empty_like(ya))) if off_out else (lambda: None)
        co = _off(torch.empty_like(ca)) if off_out else None
        _check_route(ops, key, want_vec=False, in_mod16=xi.data_ptr() % 16, out_mod16=4 if off_out else 0, symmetric=sym)
        _same(ops.int_quantize(xi, *args, out=fo()), ya, what + " quantize")
        _same(ops.int_to_integer(xi, *args, out=fo()), ta, what + " to_integer")
        _same(ops.int_encode(xi, *args, out=co), ca, what + " encode")
        _same(ops.int_decode(ci, *args, out=fo()), da, what + " decode")
        r = ops.int_range_quantize(xi, xmin, xmax, 8, sym, out=fo())
        _same(r[0], ra, what + " range_quantize")
        _same(r[1], q._delta.reshape(-1), what + " delta")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=_id)
@pytest.mark.parametrize("key", cc.UNALIGNED, ids=_id)
def test_unaligned_int_half(key, dtype):
    """x one element (2 bytes) off: the half kernels' scalar head in front of the 16-byte groups"""
    from fp8q import ops
    ref = _int_ref(key, 8, False, dtype)
    q = ref["q"]
    xg = ref["x"].cuda()
    args = _range_args(q, False) + (8, False, q.eps)
    xi = _off(xg)
    _check_route(ops, key, elem_bytes=2, in_mod16=2)
    _same(ops.int_quantize(xi, *args, out_dtype=dtype), ref["y"].to(dtype), f"{key} quantize")
    codes = ops.int_encode(xi, *args)
    _same(codes, ref["codes"], f"{key} encode")
    _same(ops.int_decode(_off(codes), *args, out_dtype=dtype), ref["dec"].to(dtype), f"{key} decode")


@pytest.mark.parametrize("fmt", ["e4m3fn", "e5m2"])
@pytest.mark.parametrize("key", cc.UNALIGNED, ids=_id)
def test_unaligned_ocp(key, fmt):
    from fp8q import ops
    case = cc.ocp_case(key, fmt)
    xg, mg = torch.from_numpy(case["x"]).cuda(), torch.from_numpy(case["maxval"]).cuda()
    ca, sa = ops.ocp_encode(xg, mg, FMT[fmt])
    ya = ops.ocp_quantize(xg, mg, FMT[fmt])
    da = ops.ocp_decode(ca, sa)
    for off_in, off_out in ((True, False), (False, True), (True, True)):
        what = f"{key} {fmt} in{'+1' if off_in else ''} out{'+1' if off_out else ''}"
        xi = _off(xg) if off_in else xg
        ci = _off(ca.view(torch.uint8)) if off_in else ca.view(torch.uint8)
        _check_route(ops, key, want_vec=False, in_mod16=xi.data_ptr() % 16, out_mod16=4 if off_out else 0)
        co = _off(torch.empty_like(ca.view(torch.uint8))) if off_out else None
        _same(ops.ocp_encode(xi, mg, FMT[fmt], out=co)[0].view(torch.uint8), ca.view(torch.uint8), what + " encode")
        _same(ops.ocp_quantize(xi, mg, FMT[fmt], out=_off(torch.empty_like(ya)) if off_out else None), ya, what + " quantize")
        _same(ops.ocp_decode(ci, sa, out=_off(torch.empty_like(da)) if off_out else None, fmt=FMT[fmt]), da, what + " decode")
