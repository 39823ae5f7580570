"""CPU-only checks of the block-scaled FP8 product (fp8q_ocpbmm_nt, ops.ocp_block_matmul): the entry is in the header, the ctypes
table and the build, and every argument error is told before anything touches a device."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3, U8, F32 = torch.float8_e4m3fn, torch.uint8, torch.float32


def test_entry_header_table_and_build():
    from fp8q import _lib, build
    hdr = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("fp8q_ocpbmm_")) == ["fp8q_ocpbmm_nt"]
    assert len(_lib.SIGNATURES["fp8q_ocpbmm_nt"][1]) == 16 and re.search(r"\bint fp8q_ocpbmm_nt\(", hdr)
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr)
    assert "fp8q_ocp_block_mm.hip" in build.SOURCES and "fp8q_mmq.h" in build.HEADERS


def test_c_refusals_before_the_launch():
    import fp8q
    mm, nul, t = fp8q.lib().fp8q_ocpbmm_nt, (None,) * 5, (1, 128, 128, 128)
    assert mm(*nul, 4, 4, 0, *t, 0, 0, 0, None) == -1                   # no K
    assert mm(*nul, -1, 4, 64, *t, 0, 0, 0, None) == -1                 # a negative M
    assert mm(*nul, 4, 4, 64, *t, 2, 0, 0, None) == -2                  # unknown format
    assert mm(*nul, 4, 4, 64, *t, 0, 2, 0, None) == -2
    assert mm(*nul, 4, 4, 64, 128, 1, 128, 128, 0, 0, 0, None) == -2    # 128x1 is the operand of no product
    assert mm(*nul, 4, 4, 64, 1, 128, 1, 64, 0, 0, 0, None) == -2       # unknown tile
    assert mm(*nul, 4, 4, 64, *t, 0, 0, 3, None) == -1                  # unknown output type
    assert mm(*nul, 0, 4, 64, *t, 0, 0, 0, None) == 0                   # an empty M or N is a no-op
    assert mm(*nul, 4, 0, 70, 128, 128, 1, 128, 1, 1, 2, None) == 0
    assert mm(*nul, 4, 4, 64, *t, 0, 0, 0, None) == -1                  # null pointers
    assert mm(4097, 4096, 4097, 4096, 4098, 4, 4, 64, *t, 0, 0, 0, None) == -1      # a float32 y off its alignment
    assert mm(4097, 4098, 4097, 4096, 4096, 4, 4, 64, *t, 0, 0, 0, None) == -1      # scales off theirs
    assert mm(4096, 4096, 4096, 4096, 4096, 65536 * 128, 4, 64, *t, 0, 0, 0, None) == -1    # a grid beyond 65535 rows of tiles


@pytest.mark.parametrize("ka, kb, kw, dtype, what", [
    (64, 96, {}, E4M3, "disagree on K"), (64, 64, {}, U8, "carry no format"), (64, 64, {"a_tile": (128, 1)}, E4M3, "a_tile must"),
    (64, 64, {"b_tile": (1, 64)}, E4M3, "b_tile must"), (64, 64, {"b_tile": (1, 128)}, E4M3, "b_scales are"),
    (64, 64, {"a_fmt": torch.float8_e5m2}, E4M3, "but a_fmt is"), (64, 64, {}, E4M3, "CUDA")])
def test_ops_refuse_before_the_device_check(ka, kb, kw, dtype, what):
    from fp8q import Fp8qError, ops
    a, b = torch.zeros(4, ka, dtype=U8).view(dtype), torch.zeros(5, kb, dtype=U8).view(dtype)
    sa, sb = torch.zeros(4, 1, dtype=F32), torch.zeros(1, 1, dtype=F32)
    with pytest.raises(Fp8qError, match=what):
        ops.ocp_block_matmul(a, sa, b, sb, **kw)
    with pytest.raises(Fp8qError, match="float32 or float16"):
        ops.ocp_block_matmul(a, sa, b, sb, out_dtype=torch.float64)
    with pytest.raises(Fp8qError, match="must be 2-D"):
        ops.ocp_block_matmul(torch.zeros(2, 2, kb, dtype=U8).view(E4M3), sa, b, sb, a_tile=(128, 128))
