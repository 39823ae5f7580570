"""The C ABI of the uniform quantizers' one-pass line search (fp8q_int_sse_grid_f32 / _f64): exports, argument errors
(all reported before any launch, so a CPU box can exercise them) and the workspace size."""
import ctypes

import pytest

EINVAL, EUNSUPPORTED, EWORKSPACE, ETOOMANY = -1, -2, -3, -5
ENTRIES = ["fp8q_int_sse_grid_f32", "fp8q_int_sse_grid_f64"]


@pytest.fixture(scope="module")
def L():
    import fp8q
    return fp8q.lib()


@pytest.fixture(scope="module")
def bufs():
    """host memory standing in for device pointers: nothing is launched when an argument is refused"""
    raw = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(raw) + 63) & ~63
    return raw, base


def _call(L, name, base, **kw):
    a = dict(x=base, C=2, inner=100, thr=base + 1024, n_cand=10, n_bits=8, symmetric=1, one_sided=0, eps=1e-8,
             out=base + 2048, ws=base + 3072, ws_bytes=1 << 30)
    a.update(kw)
    return getattr(L, name)(a["x"], a["C"], a["inner"], a["thr"], a["n_cand"], a["n_bits"], a["symmetric"],
                            a["one_sided"], a["eps"], a["out"], a["ws"], a["ws_bytes"], None)


def test_symbols_exist(L):
    import fp8q
    raw = ctypes.CDLL(fp8q.so_path())
    for name in ENTRIES + ["fp8q_int_sse_grid_workspace_bytes"]:
        assert hasattr(raw, name), name
        assert name in fp8q._lib.SIGNATURES
    assert L.fp8q_version() == 601          # additive entries


@pytest.mark.parametrize("name", ENTRIES)
def test_einval(L, bufs, name):
    _, base = bufs
    for bad in (dict(x=None), dict(thr=None), dict(out=None), dict(C=0), dict(C=-1), dict(inner=0), dict(inner=-5),
                dict(n_cand=0), dict(n_cand=-3)):
        assert _call(L, name, base, **bad) == EINVAL, bad
    elem = 4 if name.endswith("f32") else 8
    assert _call(L, name, base, x=base + elem // 2) == EINVAL       # x off its natural alignment
    assert _call(L, name, base, thr=base + 1024 + 2) == EINVAL
    assert _call(L, name, base, out=base + 2048 + 4) == EINVAL


@pytest.mark.parametrize("name", ENTRIES)
def test_eunsupported_etoomany_eworkspace(L, bufs, name):
    _, base = bufs
    for n_bits in (1, 0, -1, 17, 32):
        assert _call(L, name, base, n_bits=n_bits) == EUNSUPPORTED, n_bits
    assert _call(L, name, base, C=65536) == ETOOMANY
    need = L.fp8q_int_sse_grid_workspace_bytes(2, 100, 10)
    assert _call(L, name, base, ws=None) == EWORKSPACE
    assert _call(L, name, base, ws=base + 3072 + 4) == EWORKSPACE     # not 8-byte aligned
    assert _call(L, name, base, ws_bytes=need - 1) == EWORKSPACE
    assert _call(L, name, base, ws_bytes=0) == EWORKSPACE


def test_workspace_bytes(L):
    f = L.fp8q_int_sse_grid_workspace_bytes
    for C, inner in [(1, 1), (1, 5_000_000), (5, 4097), (64, 3000), (65535, 7)]:
        prev = 0
        for n_cand in (1, 63, 64, 65, 256, 257, 1000, 4096):
            b = f(C, inner, n_cand)
            assert b > 0 and b % 8 == 0
            assert b >= C * n_cand * 8              # at least one partial per (row, candidate)
            assert b >= prev, (C, inner, n_cand)    # monotone in n_cand
            prev = b
    assert f(0, 5, 10) > 0 and f(5, 0, 10) > 0 and f(5, 5, 0) > 0      # a floor, never zero
