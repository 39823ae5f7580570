"""C ABI of the INT quantizers' integer codes (csrc/fp8q_intcodec.hip), without a device: the three entry points exist with the
declared signatures and reject bad arguments before any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fp8q_int_to_integer_f32", "fp8q_int_encode", "fp8q_int_decode"]
EINVAL, EUNSUPPORTED = -1, -2


def test_symbols_and_signatures():
    import fp8q
    from fp8q import _lib
    hdr = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    raw = ctypes.CDLL(fp8q.so_path())
    vp, i64, i, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    for n in NAMES:
        assert hasattr(raw, n), n
        # (in, out, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps, stream) -> int
        assert _lib.SIGNATURES[n] == (i, [vp, vp, i64, i64, vp, vp, i64, vp, i, i, f, vp]), n
        decl = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\);", hdr)
        assert decl, n
        args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
        assert len(args) == 12 and args[2:] == ["int64_t C", "int64_t inner", "const float *delta", "const float *zero_float",
                                                "int64_t n_delta", "const unsigned char *signed_flag", "int n_bits",
                                                "int symmetric", "float eps", "fp8q_stream_t stream"], (n, args)
    assert re.search(r"fp8q_int_encode\s*\(const float \*x, void \*codes,", hdr)
    assert re.search(r"fp8q_int_decode\s*\(const void \*codes, float \*y,", hdr)
    assert re.search(r"fp8q_int_to_integer_f32\s*\(const float \*x, float \*t,", hdr)
    assert fp8q.lib().fp8q_version() == 601


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_without_a_device(name):
    """Every check runs before the launch, so host memory stands in for the device pointers: nothing dereferences them."""
    import fp8q
    fn = getattr(fp8q.lib(), name)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(src=p, dst=p, C=5, inner=4, delta=p, zf=p, n_delta=1, sflag=p, n_bits=8, symmetric=0):
        return fn(src, dst, C, inner, delta, zf, n_delta, sflag, n_bits, symmetric, 1e-8, None)
    assert call(src=None) == EINVAL and call(dst=None) == EINVAL and call(delta=None) == EINVAL
    assert call(zf=None, symmetric=0) == EINVAL and call(sflag=None, symmetric=1) == EINVAL
    assert call(C=0) == EINVAL and call(inner=0) == EINVAL
    assert call(C=5, n_delta=2) == EINVAL
    assert call(n_bits=1) == EUNSUPPORTED and call(n_bits=17) == EUNSUPPORTED
    if name != "fp8q_int_to_integer_f32":           # 2-byte codes at an odd address
        odd = dict(dst=p + 1) if name == "fp8q_int_encode" else dict(src=p + 1)
        assert call(n_bits=16, **odd) == EINVAL
        assert call(n_bits=17, **odd) == EUNSUPPORTED
