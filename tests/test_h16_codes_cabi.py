"""CPU-only checks of the half-precision storage-code entry points (csrc/fp8q_codec_h16.hip): every argument error is
reported before any launch, so it is exercised without a GPU; the ops wrappers and the uniform quantizers refuse what the
lane does not take.  No call here has a complete set of valid arguments: that would launch."""
import pytest

F32, F16, BF16 = 0, 1, 2
EINVAL, EUNSUPPORTED = -1, -2
P = 4096                                     # a non-null, 16-byte aligned pointer value that is never dereferenced


def test_encode_decode_h16_argument_validation_without_gpu():
    import fp8q
    L = fp8q.lib()
    # encode: (x, codes, x_type, C, inner, maxval, n_maxval, mbits, n_bits, sign_bits, stream)
    # decode: (codes, y, y_type, ...)
    for fn in (L.fp8q_encode_h16, L.fp8q_decode_h16):
        for t in (F16, BF16):
            assert fn(None, P, t, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL          # null pointers
            assert fn(P, None, t, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL
            assert fn(P, P, t, 4, 8, None, 1, 3.0, 8, 1, None) == EINVAL
            assert fn(P, P, t, 0, 8, P, 1, 3.0, 8, 1, None) == EINVAL             # empty shapes
            assert fn(P, P, t, 4, 0, P, 1, 3.0, 8, 1, None) == EINVAL
            assert fn(P, P, t, 4, -1, P, 1, 3.0, 8, 1, None) == EINVAL
            assert fn(P, P, t, 4, 8, P, 3, 3.0, 8, 1, None) == EINVAL             # n_maxval not in {1, C}
            assert fn(P, P, t, 4, 8, P, 1, 3.0, 8, 2, None) == EINVAL             # sign_bits not in {0, 1}
            assert fn(P, P, t, 4, 8, P, 1, 3.0, 9, 1, None) == EUNSUPPORTED       # a code is one byte
            assert fn(P, P, t, 4, 8, P, 4, 1.0, 16, 1, None) == EUNSUPPORTED
            assert fn(P, P, t, 4, 8, P, 1, 3.0, 4, 1, None) == EUNSUPPORTED       # sign + 3 fraction bits: no exponent bit
            assert fn(P, P, t, 4, 8, P, 1, 7.0, 7, 0, None) == EUNSUPPORTED
            # the size limits of fp8q_quantize_h16: per-channel rows beyond 2^30 elements, C * inner beyond int64, chunk counts
            assert fn(P, P, t, 2, (1 << 30) + 1, P, 2, 3.0, 8, 1, None) == EINVAL
            assert fn(P, P, t, 1 << 40, 1 << 40, P, 1, 3.0, 8, 1, None) == EINVAL
            assert fn(P, P, t, 1 << 22, 1 << 22, P, 1, 3.0, 8, 1, None) == EINVAL
        for bad in (F32, 3, -1):                                                  # not a half type
            assert fn(P, P, bad, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL
    for t in (F16, BF16):                                                         # odd address of a 2-byte element
        assert L.fp8q_encode_h16(P + 1, P, t, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL
        assert L.fp8q_decode_h16(P, P + 1, t, 4, 8, P, 1, 3.0, 8, 1, None) == EINVAL


def test_int_encode_decode_h16_argument_validation_without_gpu():
    import fp8q
    L = fp8q.lib()
    # encode: (x, codes, x_type, C, inner, delta, zero_float, n_delta, signed_flag, n_bits, symmetric, eps, stream)
    # decode: (codes, y, y_type, ...)
    for fn in (L.fp8q_int_encode_h16, L.fp8q_int_decode_h16):
        for t in (F16, BF16):
            assert fn(None, P, t, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL    # null pointers
            assert fn(P, None, t, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
            assert fn(P, P, t, 4, 8, None, P, 1, None, 8, 0, 1e-8, None) == EINVAL    # null delta
            assert fn(P, P, t, 4, 8, P, None, 1, None, 8, 0, 1e-8, None) == EINVAL    # asymmetric without zero_float
            assert fn(P, P, t, 4, 8, P, None, 1, None, 8, 1, 1e-8, None) == EINVAL    # symmetric without the sign byte
            assert fn(P, P, t, 0, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL       # empty shapes
            assert fn(P, P, t, 4, 0, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
            assert fn(P, P, t, 4, 8, P, P, 3, None, 8, 0, 1e-8, None) == EINVAL       # n_delta not in {1, C}
            assert fn(P, P, t, 4, 8, P, P, 1, None, 1, 0, 1e-8, None) == EUNSUPPORTED
            assert fn(P, P, t, 4, 8, P, None, 1, P, 17, 1, 1e-8, None) == EUNSUPPORTED
            # the size limits of fp8q_int_encode / fp8q_int_decode
            assert fn(P, P, t, 2, 1 << 31, P, P, 2, None, 8, 0, 1e-8, None) == EINVAL
            assert fn(P, P, t, 1 << 40, 1 << 40, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
            assert fn(P, P, t, 1 << 30, 1 << 30, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
        for bad in (F32, 3, -1):
            assert fn(P, P, bad, 4, 8, P, P, 1, None, 8, 0, 1e-8, None) == EINVAL
    for t in (F16, BF16):
        for n_bits in (8, 16):                                                    # odd address of a half element
            assert L.fp8q_int_encode_h16(P + 1, P, t, 4, 8, P, P, 1, None, n_bits, 0, 1e-8, None) == EINVAL
            assert L.fp8q_int_decode_h16(P, P + 1, t, 4, 8, P, P, 1, None, n_bits, 0, 1e-8, None) == EINVAL
        for n_bits in (9, 16):                                                    # ... and of a 2-byte code
            assert L.fp8q_int_encode_h16(P, P + 1, t, 4, 8, P, P, 1, None, n_bits, 0, 1e-8, None) == EINVAL
            assert L.fp8q_int_decode_h16(P + 1, P, t, 4, 8, P, P, 1, None, n_bits, 0, 1e-8, None) == EINVAL


def test_signatures_of_the_four_entries():
    from fp8q._lib import SIGNATURES
    for name in ("fp8q_encode_h16", "fp8q_decode_h16", "fp8q_int_encode_h16", "fp8q_int_decode_h16"):
        assert name in SIGNATURES
    assert len(SIGNATURES["fp8q_encode_h16"][1]) == len(SIGNATURES["fp8q_encode_u8"][1]) + 1
    assert len(SIGNATURES["fp8q_int_decode_h16"][1]) == len(SIGNATURES["fp8q_int_decode"][1]) + 1


def test_wrappers_refuse_what_the_lane_does_not_take():
    import torch
    from fp8q import ops
    from fp8q._lib import Fp8qError
    mv, d, z = torch.ones(1), torch.ones(1), torch.zeros(1)
    codes = torch.zeros(4, 8, dtype=torch.uint8)
    codes16 = torch.zeros(4, 8, dtype=torch.int16)
    for dt in (torch.float16, torch.bfloat16):
        x = torch.zeros(4, 8, dtype=dt)
        other = torch.bfloat16 if dt == torch.float16 else torch.float16
        with pytest.raises(Fp8qError, match="CUDA"):                          # half x is accepted; there is no CPU path
            ops.encode(x, mv, 3.0)
        with pytest.raises(Fp8qError, match="CUDA"):
            ops.int_encode(x, d, z)
        with pytest.raises(Fp8qError, match="CUDA"):
            ops.decode(codes, mv, 3.0, out_dtype=dt)
        with pytest.raises(Fp8qError, match="CUDA"):
            ops.int_decode(codes, d, z, out_dtype=dt)
        with pytest.raises(Fp8qError, match="CUDA"):
            ops.int_decode(codes16, d, z, n_bits=16, out=torch.empty(4, 8, dtype=dt))
        for bad in (torch.float64, torch.int8):                               # float32 or a half type only
            with pytest.raises(Fp8qError, match="float32 or"):
                ops.decode(codes, mv, 3.0, out_dtype=bad)
            with pytest.raises(Fp8qError, match="float32 or"):
                ops.int_decode(codes, d, z, out_dtype=bad)
            with pytest.raises(Fp8qError, match="float32 or"):
                ops.decode(codes, mv, 3.0, out=torch.empty(4, 8, dtype=bad))
        with pytest.raises(Fp8qError, match="float32 or"):                    # int_decode too
            ops.int_decode(codes, d, z, out=torch.empty(4, 8, dtype=torch.int8))
        with pytest.raises(Fp8qError, match="out_dtype"):                     # the other half type than `out`'s: a disagreement
            ops.decode(codes, mv, 3.0, out=torch.empty(4, 8, dtype=dt), out_dtype=other)
        with pytest.raises(Fp8qError, match="out_dtype"):
            ops.int_decode(codes, d, z, out=torch.empty(4, 8, dtype=dt), out_dtype=other)
        with pytest.raises(Fp8qError, match="out_dtype"):                     # out and out_dtype disagree
            ops.decode(codes, mv, 3.0, out=torch.empty(4, 8, dtype=dt), out_dtype=torch.float32)
        with pytest.raises(Fp8qError, match="out_dtype"):
            ops.int_decode(codes, d, z, out=torch.empty(4, 8), out_dtype=dt)
        with pytest.raises(Fp8qError):                                        # to_integer stays float32-only
            ops.int_to_integer(x, d, z)


def test_uniform_encode_needs_keep_dtype_for_half():
    import torch
    from fp8q._lib import Fp8qError
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    for cls in (AsymmetricUniformQuantizer, SymmetricUniformQuantizer):
        for keep in (False, True):
            q = cls(n_bits=8, keep_dtype=keep)
            q.set_quant_range(torch.tensor(-1.0), torch.tensor(2.0))
            for dt in (torch.float16, torch.bfloat16):
                with pytest.raises(Fp8qError, match="encode needs"):          # (with keep_dtype: still no CPU path)
                    q.encode(torch.zeros(4, 8, dtype=dt))
            with pytest.raises(Fp8qError, match="decode needs"):
                q.decode(torch.zeros(4, 8, dtype=torch.uint8), out_dtype=torch.bfloat16)
