"""CPU-only checks of the grouped MX product (fp8q_mxgmm_plan, fp8q_mxgmm_nt, ops.mx_grouped_matmul, ops.mx_grouped_plan): the
entries are in the header, the ctypes table and the build; the plan's m_tiles_max is the maximum over all count vectors, by
brute force; every argument error is told before anything touches a device."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3, U8 = torch.float8_e4m3fn, torch.uint8


def test_entries_header_table_and_build():
    from fp8q import _lib, build
    hdr = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("fp8q_mxgmm_")) == ["fp8q_mxgmm_nt", "fp8q_mxgmm_plan"]
    assert len(_lib.SIGNATURES["fp8q_mxgmm_nt"][1]) == 18 and len(_lib.SIGNATURES["fp8q_mxgmm_plan"][1]) == 6
    assert re.search(r"\bint fp8q_mxgmm_nt\(", hdr) and re.search(r"\bint fp8q_mxgmm_plan\(", hdr)
    assert "fp8q_mx_mm_grouped.hip" in build.SOURCES and "fp8q_mx_mm_grouped.hip" in build.EXTRA_CFLAGS


@pytest.mark.parametrize("TM", [2, 3])
def test_m_tiles_max_is_the_maximum_over_all_counts(TM):
    """The rule (T - n) / TM + n, n = min(G, T), and 0 for n == 0, against every count vector with sum <= T, at tile heights
    small enough to enumerate; the C plan at its own heights is the same expression."""
    from fp8q import ops
    for T, G in itertools.product(range(0, 8), range(0, 5)):
        best = max(sum(-(-c // TM) for c in counts) for counts in itertools.product(range(T + 1), repeat=G) if sum(counts) <= T)
        n = min(G, T)
        assert best == ((T - n) // TM + n if n else 0), (T, G)
    for T, G in [(0, 3), (5, 0), (1, 1), (64, 32), (295, 7), (512, 32), (1025, 32), (8192, 32), (40, 4096)]:
        n = min(G, T)
        for tm in (32, 128):
            tiles = (T - n) // tm + n if n else 0
            assert ops.mx_grouped_plan(T, 129, 64, G, tm) == (tm, tiles, 8 * tiles)
        assert ops.mx_grouped_plan(T, 129, 64, G)[0] == (32 if T <= 32 * n else 128)


def test_c_refusals_before_the_launch():
    import ctypes
    import fp8q
    mm, plan, p3 = fp8q.lib().fp8q_mxgmm_nt, fp8q.lib().fp8q_mxgmm_plan, (ctypes.c_int64 * 3)()

    def call(T=4, N=4, K=64, G=2, fa=0, fb=0, yt=0, tile=0, ptr=4096, off=4096, y=4096, ws=4096, wsb=64):
        return mm(ptr, ptr, ptr, ptr, off, 0, y, T, N, K, G, fa, fb, yt, tile, ws, wsb, None)

    assert call(fa=3) == -2 and call(G=4097) == -2 and call(tile=64) == -2      # format 3 is unassigned
    assert call(K=48) == -1 and call(yt=3) == -1 and call(T=1 << 31) == -1
    assert call(T=65536 * 128, G=1, tile=128) == -1                             # m_tiles_max = 65536
    assert call(T=0, ptr=None) == 0 and call(N=0, ptr=None) == 0 and call(G=0, ptr=None) == 0     # empty: a no-op
    assert call(ptr=None) == -1 and call(off=None) == -1 and call(y=4098) == -1 and call(off=4098) == -1
    assert plan(4, 4, 64, 2, 0, p3) == 0 and list(p3) == [32, 2, 16]
    assert call(ws=None) == -1 and call(wsb=15) == -1 and call(ws=4104) == -1   # a null, small or misaligned workspace
    assert plan(4, 4, 64, 4097, 0, p3) == -2 and plan(4, 4, 48, 2, 0, p3) == -1 and plan(4, 4, 64, 2, 0, None) == -1


def test_ops_refuse_before_the_device_check():
    from fp8q import Fp8qError, ops

    def call(T=4, G=2, off=None, bdim3=True, **kw):
        a, b = torch.zeros(T, 64, dtype=U8).view(E4M3), torch.zeros(G, 5, 64, dtype=U8).view(E4M3)
        off = torch.zeros(G + 1, dtype=torch.int32) if off is None else off
        return ops.mx_grouped_matmul(a, torch.zeros(T, 2, dtype=U8), b if bdim3 else b[0], torch.zeros(G, 5, 2, dtype=U8), off,
                                     **kw)

    with pytest.raises(Fp8qError, match="tile_m must be"):
        call(tile_m=64)
    with pytest.raises(Fp8qError, match="3-D"):
        call(bdim3=False)
    with pytest.raises(Fp8qError, match="offsets are"):
        call(off=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(Fp8qError, match="float32 or float16"):
        call(out_dtype=torch.float64)
    with pytest.raises(Fp8qError, match="G <= 4096"):
        call(G=4097)
    with pytest.raises(Fp8qError, match="CUDA"):                # a good call gets as far as the device check
        call(tile_m=32)
