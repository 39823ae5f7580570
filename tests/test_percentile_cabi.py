"""C ABI of the percentile selection (csrc/fp8q_select.hip), without a device: the three entry points exist with the declared
signatures and reject bad arguments before any HIP call."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fp8q_percentile_resident_max_inner", "fp8q_percentile_workspace_bytes", "fp8q_percentile_f32"]
EINVAL = -1


def test_symbols_and_signatures():
    import fp8q
    from fp8q import _lib
    hdr = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    raw = ctypes.CDLL(fp8q.so_path())
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in _lib.SIGNATURES, n
    vp, i64, i, d, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    assert _lib.SIGNATURES["fp8q_percentile_resident_max_inner"] == (i64, [])
    assert _lib.SIGNATURES["fp8q_percentile_workspace_bytes"] == (sz, [i64, i64])
    assert _lib.SIGNATURES["fp8q_percentile_f32"] == (i, [vp, i64, i64, d, vp, vp, vp, sz, vp])
    assert re.search(r"\bint64_t\s+fp8q_percentile_resident_max_inner\s*\(void\);", hdr)
    assert re.search(r"\bsize_t\s+fp8q_percentile_workspace_bytes\s*\(int64_t C, int64_t inner\);", hdr)
    decl = re.search(r"\bint\s+fp8q_percentile_f32\s*\(([^;]*)\);", hdr)
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert args == ["const float *x", "int64_t C", "int64_t inner", "double pct", "float *lo", "float *hi", "void *ws",
                    "size_t ws_bytes", "fp8q_stream_t stream"], args
    assert fp8q.lib().fp8q_version() == 601
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr)


def test_argument_errors_without_a_device():
    """Every check runs before any HIP call, so host memory stands in for the device pointers: nothing dereferences them."""
    import fp8q
    L = fp8q.lib()
    R = L.fp8q_percentile_resident_max_inner()
    assert R >= 4608                       # the per-channel weight shapes ([C,512,3,3]) are row-resident
    buf = (ctypes.c_double * 64)()         # 8-byte aligned
    p = ctypes.addressof(buf)
    big = 1 << 40                          # "large enough" for every shape below (never touched)

    def call(x=p, C=3, inner=100, pct=1.0, lo=p, hi=p, ws=p, ws_bytes=big):
        return L.fp8q_percentile_f32(x, C, inner, pct, lo, hi, ws, ws_bytes, None)
    assert call(x=None) == EINVAL and call(lo=None) == EINVAL and call(hi=None) == EINVAL
    assert call(C=0) == EINVAL and call(C=-1) == EINVAL and call(inner=0) == EINVAL and call(inner=-5) == EINVAL
    assert call(pct=float("nan")) == EINVAL and call(pct=-1e-9) == EINVAL and call(pct=100.0000001) == EINVAL
    assert call(pct=float("inf")) == EINVAL
    # the streaming route needs its workspace: present, 8-byte aligned, large enough
    need = L.fp8q_percentile_workspace_bytes(3, R + 1)
    assert need > 0
    assert call(inner=R + 1, ws=None, ws_bytes=0) == EINVAL
    assert call(inner=R + 1, ws=p + 4) == EINVAL
    assert call(inner=R + 1, ws_bytes=need - 1) == EINVAL
    assert call(inner=R + 1, ws_bytes=0) == EINVAL
    # bad arguments win over a missing workspace, on both routes
    assert call(inner=R + 1, pct=101.0, ws=None, ws_bytes=0) == EINVAL
    assert call(inner=R, x=None, ws=None, ws_bytes=0) == EINVAL


def test_workspace_bytes_are_monotone_and_8_byte_granular():
    import fp8q
    L = fp8q.lib()
    R = L.fp8q_percentile_resident_max_inner()
    f = L.fp8q_percentile_workspace_bytes
    inners = [1, 2, 147, 4608, R, R + 1, 2 * R + 3, 70001, (1 << 20) + 77, (1 << 24) + 1, 64 * 112 * 112 * 64]
    Cs = [1, 2, 3, 64, 1025, 58254]
    for C in Cs:
        row = [f(C, n) for n in inners]
        assert all(v % 8 == 0 for v in row), (C, row)
        assert all(a <= b for a, b in zip(row, row[1:])), (C, row)
        assert all(f(C, n) == 0 for n in inners if n <= R), C       # the row-resident route needs none
        assert all(f(C, n) > 0 for n in inners if n > R), C
    for n in inners:
        col = [f(C, n) for C in Cs]
        assert all(a <= b for a, b in zip(col, col[1:])), (n, col)
    assert all(f(C, R + 1) < f(C2, R + 1) for C, C2 in zip(Cs, Cs[1:]))
