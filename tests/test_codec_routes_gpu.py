"""The storage-code kernels on the GPU at every shape of tests/codec_cases.py, through the C entry points: the route from the REAL
pointers' phases first (ops.codec_route), then the whole output against the CPU oracle on integers -- codes as uint8, decoded
values with identical NaN masks and identical int32 bits elsewhere, the sign of zero included; no tolerance, no sampled subset.
Every input and output is a window inside a sentinel-filled buffer whose guard elements are checked unchanged."""
import numpy as np
import pytest
import torch

import codec_cases as cc
import epilogue_cases as ec
import oracle
import rows_cases as rc
from epilogue_cases import same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
F_SENTINEL = 7.0
C_SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ops():
    from fp8q import ops as o
    assert torch.cuda.is_available()
    return o


def _keys():
    from fp8q import ops as o
    return sorted(cc.build_shapes(o).items(), key=lambda kv: repr(kv[0]))


KEYS = _keys()
_refs = {}


def _ref(key):
    """(case, oracle codes, oracle values of those codes) of a key's input: computed once, shared by both directions and all
    phases, left unchanged"""
    ck = (key[1], key[2], key[3], key[6])
    if ck not in _refs:
        if key[1] * key[2] > cc.BIG:
            _refs.clear()                # (one large reference at a time)
        case = cc.case_input(key)
        codes = oracle.c_encode(case["x"], case["maxval"], *key[3])
        _refs[ck] = (case, codes, oracle.c_decode(codes, case["maxval"], *key[3]))
    return _refs[ck]


def _fwindow(n, phase):
    """(buffer, an n-element float32 window `phase` elements behind a 16-byte boundary, its offset): GUARD sentinels and more around it"""
    buf = torch.full((n + 2 * GUARD + 8,), F_SENTINEL, dtype=torch.float32, device="cuda")
    off = GUARD + (phase - (buf.data_ptr() // 4 + GUARD)) % 4
    win = buf[off:off + n]
    assert win.data_ptr() % 16 == 4 * phase
    return buf, win, off


def _cwindow(n, phase):
    """the same for codes: uint8, `phase` bytes behind a 16-byte boundary"""
    buf = torch.full((n + 2 * GUARD + 32,), C_SENTINEL, dtype=torch.uint8, device="cuda")
    off = GUARD + (phase - (buf.data_ptr() + GUARD)) % 16
    win = buf[off:off + n]
    assert win.data_ptr() % 16 == phase
    return buf, win, off


def _guards_intact(buf, off, n, sentinel):
    c = buf.cpu()
    return bool((c[:off] == sentinel).all()) and bool((c[off + n:] == sentinel).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _assert_route(ops, key, want, fwin, cwin):
    enc, C, inner, fmt, _, _, pc = key
    got = ops.codec_route(enc, C, inner, pc, *fmt, fp_mod16=fwin.data_ptr() % 16, code_mod16=cwin.data_ptr() % 16)
    assert all(got[k] == v for k, v in want.items()), (key, want, got)
    return got


def _encode(fmt, x, codes, C, inner, mv):
    from fp8q._lib import check, lib
    check(lib().fp8q_encode_u8(x.data_ptr(), codes.data_ptr(), C, inner, mv.data_ptr(), mv.numel(), float(fmt[0]), fmt[1], fmt[2],
                               _stream()), "fp8q_encode_u8")


def _decode(fmt, codes, y, C, inner, mv):
    from fp8q._lib import check, lib
    check(lib().fp8q_decode_u8(codes.data_ptr(), y.data_ptr(), C, inner, mv.data_ptr(), mv.numel(), float(fmt[0]), fmt[1], fmt[2],
                               _stream()), "fp8q_decode_u8")


def _run_encode(ops, key, want, xh, mvh, ref):
    enc, C, inner, fmt, fp, cp, pc = key
    n = C * inner
    xbuf, x, xoff = _fwindow(n, fp)
    x.copy_(torch.from_numpy(xh.reshape(-1)))
    cbuf, codes, coff = _cwindow(n, cp)
    got = _assert_route(ops, (True,) + key[1:], want, x, codes)
    _encode(fmt, x, codes, C, inner, torch.from_numpy(mvh).cuda())
    out = codes.cpu().numpy().reshape(C, inner)
    assert np.array_equal(out, ref), (key, int((out != ref).sum()), np.argwhere(out != ref)[:4])
    assert _guards_intact(cbuf, coff, n, C_SENTINEL), key
    assert _guards_intact(xbuf, xoff, n, F_SENTINEL) and np.array_equal(x.cpu().numpy().view(np.int32), xh.reshape(-1).view(np.int32)), key
    return got


def _run_decode(ops, key, want, ch, mvh, ref):
    enc, C, inner, fmt, fp, cp, pc = key
    n = C * inner
    cbuf, codes, coff = _cwindow(n, cp)
    codes.copy_(torch.from_numpy(ch.reshape(-1)))
    ybuf, y, yoff = _fwindow(n, fp)
    got = _assert_route(ops, (False,) + key[1:], want, y, codes)
    _decode(fmt, codes, y, C, inner, torch.from_numpy(mvh).cuda())
    assert same_bits(y.cpu().numpy().reshape(C, inner), ref), key
    assert _guards_intact(ybuf, yoff, n, F_SENTINEL), key
    assert _guards_intact(cbuf, coff, n, C_SENTINEL) and np.array_equal(codes.cpu().numpy(), ch.reshape(-1)), key
    return got


@pytest.mark.parametrize("key,want", [kv for kv in KEYS if kv[0][0]], ids=lambda v: repr(v) if isinstance(v, tuple) else "")
def test_encode_reaches_its_kernel_and_matches_the_oracle(ops, key, want):
    case, codes, _ = _ref(key)
    _run_encode(ops, key, want, case["x"], case["maxval"], codes)


@pytest.mark.parametrize("key,want", [kv for kv in KEYS if not kv[0][0]], ids=lambda v: repr(v) if isinstance(v, tuple) else "")
def test_decode_reaches_its_kernel_and_matches_the_oracle(ops, key, want):
    """the oracle's codes of the case's input: what the encode of the same case must have produced"""
    case, codes, vals = _ref(key)
    _run_decode(ops, key, want, codes, case["maxval"], vals)


# every valid code in every row: (C, k of all_codes, fp32 phase in elements, code phase in bytes, per channel) -> kernel
ALL_CODES = [(9, 3, 0, 0, True, "k_rows_flat"), (9, 3, 0, 4, True, "k_rows_flat"), (9, 3, 1, 0, True, "k_codec_rows"),
             (9, 3, 0, 1, True, "k_codec_rows"), (5, 3, 0, 0, False, "k_codec_rows"), (5, 3, 0, 4, False, "k_codec_rows"),
             (5, 3, 3, 7, False, "k_codec_rows"), (3, 9, 0, 0, True, None)]


@pytest.mark.parametrize("fmt", cc.FORMATS, ids=repr)
def test_every_code_decodes_and_its_value_encodes_like_the_oracle(ops, fmt):
    """Codes the encoder never emits from in-range data -- above the range's top code, every subnormal -- through both kernels at
    ranges of every kind, then the decoded values back through encode.  code -> value -> code is NOT asserted to be the identity
    (the oracle lacks it at denormal ranges): both steps are compared with the oracle's."""
    R = ec.ranges(fmt)
    for C, k, fp, cp, pc, kernel in ALL_CODES:
        ch = cc.all_codes(fmt, C, k)
        inner = ch.shape[1]
        if kernel is None:          # rows of 2048 elements and more where the format has them; else the flat kernel's tables at their limit
            kernel = "k_codec_rows" if inner >= 2048 else "k_rows_flat"
        if kernel == "k_rows_flat" and inner < cc.flat_min_inner(ops, fmt):
            kernel = "k_codec_rows"          # (eight codes: rows of 24)
        mvh = np.array([R[r % len(R)] for r in range(C)] if pc else R[:1], np.float32)
        vals = oracle.c_decode(ch, mvh, *fmt)
        key = (False, C, inner, fmt, fp, cp, pc)
        _run_decode(ops, key, dict(kernel=kernel), ch, mvh, vals)
        _run_encode(ops, key, dict(kernel=kernel), vals, mvh, oracle.c_encode(vals, mvh, *fmt))


@pytest.mark.parametrize("fmt", [cc.E4M3, cc.E7], ids=repr)
@pytest.mark.parametrize("C,inner,kernel", [(120, 147, "k_rows_flat"), (9, 2048, "k_codec_rows")])
def test_values_next_to_ties_take_the_exact_quotient(ops, fmt, C, inner, kernel):
    """rows of values within a few ulp of every tie at ranges whose bias is no integer: the fast quotient lands on the other side of
    some ties, the kernel must redo those by division (encode_group4 -> encode_one) and give the oracle's code"""
    xh, mvh = rc.tie_cloud(fmt, C, inner, C + inner)
    key = (True, C, inner, fmt, 0, 0, True)
    _run_encode(ops, key, dict(kernel=kernel), xh, mvh, oracle.c_encode(xh, mvh, *fmt))


def test_the_python_wrappers_write_into_out_views(ops):
    """ops.encode / ops.decode with out= views at a code phase of 4 and of 1: the result IS the view and equals the direct call's"""
    key = cc._k(True, 120, 147)
    C, inner, fmt = key[1:4]
    case, ref_codes, ref_vals = _ref(key)
    n = C * inner
    x = torch.from_numpy(case["x"]).cuda()
    mv = torch.from_numpy(case["maxval"]).cuda()
    for cp, kernel, wide in ((4, "k_rows_flat", False), (1, "k_codec_rows", False)):
        cbuf, codes, coff = _cwindow(n, cp)
        assert x.data_ptr() % 16 == 0
        _assert_route(ops, key, dict(kernel=kernel, wide=wide), x, codes)
        out = ops.encode(x, mv, *fmt, out=codes.view(C, inner))
        assert out.data_ptr() == codes.data_ptr() and out.shape == (C, inner)
        direct = torch.empty(n, dtype=torch.uint8, device="cuda")
        _encode(fmt, x, direct, C, inner, mv)
        assert torch.equal(codes, direct) and np.array_equal(codes.cpu().numpy().reshape(C, inner), ref_codes)
        assert _guards_intact(cbuf, coff, n, C_SENTINEL)
        ybuf, y, yoff = _fwindow(n, 0)
        yo = ops.decode(codes.view(C, inner), mv, *fmt, out=y.view(C, inner))
        assert yo.data_ptr() == y.data_ptr()
        yd = torch.empty(n, dtype=torch.float32, device="cuda")
        _decode(fmt, codes, yd, C, inner, mv)
        assert same_bits(y.cpu().numpy(), yd.cpu().numpy()) and same_bits(y.cpu().numpy().reshape(C, inner), ref_vals)
        assert _guards_intact(ybuf, yoff, n, F_SENTINEL)
