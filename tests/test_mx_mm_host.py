"""CPU-only checks of the MX product (fp8q_mxmm_nt, ops.mx_matmul): the entry is in the header, the ctypes table and the build,
and every argument error is told before anything touches a device."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3, U8 = torch.float8_e4m3fn, torch.uint8


def test_entry_header_table_and_build():
    from fp8q import _lib, build
    hdr = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("fp8q_mxmm_")) == ["fp8q_mxmm_nt"]
    assert len(_lib.SIGNATURES["fp8q_mxmm_nt"][1]) == 12 and re.search(r"\bint fp8q_mxmm_nt\(", hdr)
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr)
    assert "fp8q_mx_mm.hip" in build.SOURCES


def test_c_refusals_before_the_launch():
    import fp8q
    mm, nul = fp8q.lib().fp8q_mxmm_nt, (None,) * 5
    assert mm(*nul, 4, 4, 48, 0, 0, 0, None) == -1      # K % 32
    assert mm(*nul, 4, 4, 0, 0, 0, 0, None) == -1       # no K
    assert mm(*nul, 4, 4, 64, 3, 0, 0, None) == -2      # format 3 is unassigned
    assert mm(*nul, 4, 4, 64, 0, 6, 0, None) == -2      # unknown format
    assert mm(*nul, 4, 4, 64, 0, 0, 3, None) == -1      # unknown output type
    assert mm(*nul, 0, 4, 64, 0, 0, 0, None) == 0       # an empty M or N is a no-op
    assert mm(*nul, 4, 0, 64, 5, 2, 2, None) == 0
    assert mm(*nul, 4, 4, 64, 0, 0, 0, None) == -1      # null pointers
    assert mm(4096, 4096, 4096, 4096, 4098, 4, 4, 64, 0, 0, 0, None) == -1      # a float32 y off its alignment


@pytest.mark.parametrize("ka, kb, fmt, dtype, what", [
    (64, 96, None, E4M3, "disagree on K"), (48, 48, None, E4M3, "multiple of 32"), (64, 64, None, U8, "carry no format"),
    (64, 64, "e2m3", U8, "multiple of 3"), (64, 64, torch.float8_e5m2, E4M3, "but a_fmt is"), (64, 64, None, E4M3, "CUDA")])
def test_ops_refuse_before_the_device_check(ka, kb, fmt, dtype, what):
    from fp8q import Fp8qError, ops
    a, b = torch.zeros(4, ka, dtype=U8).view(dtype), torch.zeros(5, kb, dtype=U8).view(dtype)
    sa, sb = torch.zeros(4, ka // 32, dtype=U8), torch.zeros(5, kb // 32, dtype=U8)
    with pytest.raises(Fp8qError, match=what):
        ops.mx_matmul(a, sa, b, sb, a_fmt=fmt, b_fmt=fmt)
    with pytest.raises(Fp8qError, match="float32 or float16"):
        ops.mx_matmul(a, sa, b, sb, out_dtype=torch.float64)
