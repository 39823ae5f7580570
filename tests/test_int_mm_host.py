"""CPU-only checks of the INT product (fp8q_i8mm_nt, ops.int_matmul): the entry is in the header, the ctypes table and the build,
and every argument error is told before anything touches a device."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, F32 = torch.uint8, torch.float32


def test_entry_header_table_and_build():
    from fp8q import _lib, build
    hdr = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("fp8q_i8mm_")) == ["fp8q_i8mm_nt"]
    assert len(_lib.SIGNATURES["fp8q_i8mm_nt"][1]) == 21 and re.search(r"\bint fp8q_i8mm_nt\(", hdr)
    assert re.search(r"#define FP8Q_VERSION 601\b", hdr)
    assert "fp8q_int_mm.hip" in build.SOURCES and "fp8q_mmq.h" in build.HEADERS


def test_c_refusals_before_the_launch():
    import fp8q
    mm = fp8q.lib().fp8q_i8mm_nt
    P = 4096                                                    # a pointer that is never followed

    def side(codes=P, delta=P, zf=P, flag=None, n_delta=1, n_bits=8, sym=0):
        return (codes, delta, zf, flag, n_delta, n_bits, sym)

    def call(a=side(), b=side(), y=P, M=4, N=4, K=64, y_type=0):
        return mm(*a, *b, y, M, N, K, 1e-8, y_type, None)

    assert call(a=side(n_bits=9)) == -2 and call(b=side(n_bits=1)) == -2       # two-byte codes, one bit
    assert call(K=0) == -1 and call(M=-1) == -1                                 # no K, a negative M
    assert call(K=32769) == -2 and call(a=side(codes=None), K=32769) == -2      # T would not fit int32
    assert call(y_type=3) == -1                                                 # unknown output type
    assert call(a=side(codes=None, delta=None), M=0) == 0 and call(N=0) == 0    # an empty M or N is a no-op
    assert call(a=side(codes=None)) == -1 and call(b=side(delta=None)) == -1 and call(y=None) == -1    # null pointers
    assert call(a=side(zf=None)) == -1 and call(b=side(zf=None, sym=1)) == -1   # what the operand's kind reads
    assert call(a=side(n_delta=3)) == -1 and call(b=side(n_delta=5)) == -1      # a delta count that is neither 1 nor the rows
    assert call(a=side(delta=P + 2)) == -1 and call(y=P + 2) == -1              # delta, y off their alignment
    assert call(M=65536 * 128) == -1                                            # a grid beyond 65535 rows of tiles


@pytest.mark.parametrize("ka, kb, kw, what", [
    (64, 96, {}, "disagree on K"), (64, 64, {"a_n_bits": 9}, "a_n_bits must"), (64, 64, {"b_n_bits": 1}, "b_n_bits must"),
    (64, 64, {"a_delta": torch.ones(3)}, "a_delta are"), (64, 64, {"b_delta": torch.ones(2, 2)}, "b_delta are"),
    (0, 0, {}, "K must be in"), (32769, 32769, {}, "K must be in"), (64, 64, {"out_dtype": torch.float64}, "float32 or float16"),
    (64, 64, {"a_codes": torch.zeros(4, 64, dtype=torch.int16)}, "a_codes must be uint8"),
    (64, 64, {"b_codes": torch.zeros(2, 5, 64, dtype=U8)}, "must be 2-D"),
    (64, 64, {"a_codes": torch.zeros(2, 2, 64, dtype=U8), "a_delta": torch.ones(2)}, "per-channel a_delta"),
    (64, 64, {}, "CUDA")])
def test_ops_refuse_before_the_device_check(ka, kb, kw, what):
    from fp8q import Fp8qError, ops
    args = {"a_codes": torch.zeros(4, ka, dtype=U8), "a_delta": torch.ones(1), "b_codes": torch.zeros(5, kb, dtype=U8),
            "b_delta": torch.ones(5), "a_zero_float": torch.zeros(1), "b_zero_float": torch.zeros(5)}
    args.update(kw)
    with pytest.raises(Fp8qError, match=what):
        ops.int_matmul(args.pop("a_codes"), args.pop("a_delta"), args.pop("b_codes"), args.pop("b_delta"), **args)
