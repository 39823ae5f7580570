"""CPU-only checks of the small-M MX product (fp8q_mxsk_plan, fp8q_mxsk_nt, ops.mx_matmul(skinny=True), ops.mx_skinny_plan): the
entries are in the header, the ctypes table and the build; the plan's invariants hold by brute force (not its two tuning
constants); every argument error is told before anything touches a device."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3, U8 = torch.float8_e4m3fn, torch.uint8


def test_entries_header_table_and_build():
    from fp8q import _lib, build
    hdr = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("fp8q_mxsk_")) == ["fp8q_mxsk_nt", "fp8q_mxsk_plan"]
    assert len(_lib.SIGNATURES["fp8q_mxsk_nt"][1]) == 15 and len(_lib.SIGNATURES["fp8q_mxsk_plan"][1]) == 5
    assert re.search(r"\bint fp8q_mxsk_nt\(", hdr) and re.search(r"\bint fp8q_mxsk_plan\(", hdr)
    assert "fp8q_mx_mm_skinny.hip" in build.SOURCES


@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_plan_invariants(M):
    from fp8q import ops
    for N in (1, 64, 65, 4096, 28672):
        for K in range(32, 4097, 32):
            nsteps = -(-K // 128)
            for req in (0, 1, 2, 3, 7, 1000):
                S, T, tw, ws = ops.mx_skinny_plan(M, N, K, req or None)
                assert 1 <= S <= nsteps and (req != 1 or S == 1) and (req == 0 or S <= req), (N, K, req)
                assert ws == (0 if S == 1 else S * M * N * 4)
                # the kernel's ranges: split s owns [s T, s T + T), wave w of it tw steps from s T + w tw, clipped to both
                steps = []
                for s in range(S):
                    end = min(nsteps, (s + 1) * T)
                    assert s * T < end, "no split is empty"
                    for w in range(4):
                        k0 = min(end, s * T + w * tw)
                        steps += range(k0, min(end, k0 + tw))
                assert steps == list(range(nsteps)), (N, K, req)


def test_c_refusals_before_the_launch():
    import ctypes
    import fp8q
    mm, plan, nul, p4 = fp8q.lib().fp8q_mxsk_nt, fp8q.lib().fp8q_mxsk_plan, (None,) * 5, (ctypes.c_int64 * 4)()
    assert mm(*nul, 65, 4, 64, 0, 0, 0, 0, None, 0, None) == -2     # M > 64
    assert mm(*nul, 4, 4, 64, 3, 0, 0, 0, None, 0, None) == -2      # format 3 is unassigned
    assert mm(*nul, 4, 4, 48, 0, 0, 0, 0, None, 0, None) == -1      # K % 32
    assert mm(*nul, 4, 4, 64, 0, 0, 3, 0, None, 0, None) == -1      # unknown output type
    assert mm(*nul, 0, 4, 64, 0, 0, 0, 0, None, 0, None) == 0       # an empty M or N is a no-op
    assert mm(*nul, 4, 0, 64, 5, 2, 2, 0, None, 0, None) == 0
    assert mm(*nul, 4, 4, 64, 0, 0, 0, 0, None, 0, None) == -1      # null pointers
    ptr = (4096,) * 5
    assert mm(4096, 4096, 4096, 4096, 4098, 4, 4, 64, 0, 0, 0, 0, None, 0, None) == -1     # a float32 y off its alignment
    assert plan(4, 4, 256, 2, p4) == 0 and list(p4) == [2, 1, 1, 2 * 4 * 4 * 4]
    assert mm(*ptr, 4, 4, 256, 0, 0, 0, 2, None, 128, None) == -1       # two splits: a null workspace,
    assert mm(*ptr, 4, 4, 256, 0, 0, 0, 2, 4096, 127, None) == -1       # a smaller one than planned,
    assert mm(*ptr, 4, 4, 256, 0, 0, 0, 2, 4104, 128, None) == -1       # one off its 16-byte alignment
    assert plan(65, 4, 64, 0, p4) == -2 and plan(4, 4, 48, 0, p4) == -1 and plan(4, 4, 64, 0, None) == -1


def test_ops_refuse_before_the_device_check():
    from fp8q import Fp8qError, ops

    def call(M, **kw):
        a, b = torch.zeros(M, 64, dtype=U8).view(E4M3), torch.zeros(5, 64, dtype=U8).view(E4M3)
        return ops.mx_matmul(a, torch.zeros(M, 2, dtype=U8), b, torch.zeros(5, 2, dtype=U8), skinny=True, **kw)

    with pytest.raises(Fp8qError, match="M <= 64"):
        call(65)
    with pytest.raises(Fp8qError, match="splits must be"):
        call(4, splits=0)
    with pytest.raises(Fp8qError, match="float32 or float16"):
        call(4, out_dtype=torch.float64)
    with pytest.raises(Fp8qError, match="CUDA"):     # a good call gets as far as the device check
        call(64, splits=2)
