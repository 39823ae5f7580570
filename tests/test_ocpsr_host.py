"""CPU-only checks of the hardware FP8 lanes' stochastic rounding (the fp8q_ocpsr_* / fp8q_ocpbsr_* / fp8q_ocpbtsr_* entries,
seed= / offset= on the six ops, stochastic=True on the two quantizers): the oracle of tests/ocpsr_oracle.py against values
written down by hand, the header and the ctypes table, argument errors at the C ABI before any launch and in Python before the
device check, the quantizers' bookkeeping, and the frequency bound on the oracle alone (tests/test_ocpsr_gpu.py asserts the
same bound, with the same seeds, on the kernels)."""
import ctypes
import math
import os
import re

import pytest
import torch

import mxsr_oracle as sro
import ocpsr_oracle as oo
from ocpsr_oracle import E4M3, E5M2, FMAX, FMTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> its round-to-nearest-even twin
TWINS = {"fp8q_ocpsr_encode": "fp8q_ocp_encode", "fp8q_ocpsr_quantize": "fp8q_ocp_quantize",
         "fp8q_ocpbsr_encode": "fp8q_ocpb_encode", "fp8q_ocpbsr_quantize": "fp8q_ocpb_quantize",
         "fp8q_ocpbtsr_encode": "fp8q_ocpbt_encode", "fp8q_ocpbtsr_encode_both": "fp8q_ocpbt_encode_both"}
ENTRIES = sorted(k + sfx for k in TWINS for sfx in ("_f32", "_h16"))
F32, F16, BF16 = 0, 1, 2
_ids = [oo.NAME[f] for f in FMTS]

# ---- the frequency case, shared with tests/test_ocpsr_gpu.py ----
FREQ_N = 1 << 20
FREQ_SEEDS = (2024, 2025)           # consecutive: a quantizer built with stochastic=True, seed=2024 draws them call by call
# name: (format, the constant, its lower neighbour, its upper one, p); maxval = fmax, so scale = 1 exactly
FREQ = {"normal": (E4M3, 2.0625, 2.0, 2.25, 0.25),                         # a quarter up the step from 2 to 2.25
        "subnormal": (E4M3, 2.5 * 2.0 ** -9, 2 * 2.0 ** -9, 3 * 2.0 ** -9, 0.5)}    # below 2^-6, step 2^-9


def freq_input(name):
    return torch.full((FREQ_N // 1024, 1024), FREQ[name][1], dtype=torch.float32)


def freq_check(values, name, what):
    """values: float32, FREQ_N elements, on the CPU.  Every element is one of the two neighbours and the share that went away
    from zero lies within 5 standard deviations of p, 5 * sqrt(p (1 - p) / N) with N = 2^20 independent draws (0.0021 for
    p = 1/4): the binomial law, not tuned; the 2^-16 granularity of p is far below it"""
    _, _, lo, hi, p = FREQ[name]
    up = values == hi
    assert (up | (values == lo)).all(), f"{what}: a result that is neither neighbour"
    n = values.numel()
    assert n == FREQ_N
    share = up.sum().item() / n
    bound = 5 * math.sqrt(p * (1 - p) / n)
    print(f"{what}: share {share:.6f}, p {p}, bound {bound:.6f}")
    assert abs(share - p) <= bound, f"{what}: share {share} against p = {p} +- {bound}"
    return up


# ---- SR by hand ----
def _code(q_bits, r, fmt):
    q = torch.tensor([q_bits], dtype=torch.int32).view(torch.float32)
    one = torch.ones(1)
    pos = oo.codes_of(q, one, fmt, torch.tensor([r])).item()
    neg = oo.codes_of(-q, one, fmt, torch.tensor([r])).item()
    assert neg == pos | 0x80                  # the sign is kept and changes nothing else
    return pos


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_sr_codes_written_down_by_hand(fmt):
    M = sro.MBITS[fmt]
    sh = 23 - M
    # normal range: 2.0 is the code 0x40 in both formats, its upper neighbour (2.25 / 2.5) 0x41; f16 are the 16 bits under
    # the kept mantissa, and the code goes up exactly when f16 + r carries out of 16 bits
    base = 0x40000000
    want = {0x0000: {0: 0x40, 0x7FFF: 0x40, 0x8000: 0x40, 0xFFFF: 0x40},
            0x8000: {0: 0x40, 0x7FFF: 0x40, 0x8000: 0x41, 0xFFFF: 0x41},
            0xFFFF: {0: 0x40, 0x7FFF: 0x41, 0x8000: 0x41, 0xFFFF: 0x41}}
    for f16, by_r in want.items():
        for r, code in by_r.items():
            assert _code(base + (f16 << (sh - 16)), r, fmt) == code, (hex(f16), hex(r))
            # the bits under f16 are dropped: all of them set changes nothing
            assert _code(base + (f16 << (sh - 16)) + (1 << (sh - 16)) - 1, r, fmt) == code, (hex(f16), hex(r))
    # format-subnormal range: twice the smallest subnormal is the code 0x02, its neighbour 0x03; |q| is taken in units of
    # 2^-16 of the grid's step, 2^-25 for E4M3FN (step 2^-9) and 2^-32 for E5M2 (step 2^-16)
    step = 2.0 ** -9 if fmt == E4M3 else 2.0 ** -16
    want = {0x0000: {0: 0x02, 0x7FFF: 0x02, 0x8000: 0x02, 0xFFFF: 0x02},
            0x8000: {0: 0x02, 0x7FFF: 0x02, 0x8000: 0x03, 0xFFFF: 0x03},
            0xFFFF: {0: 0x02, 0x7FFF: 0x03, 0x8000: 0x03, 0xFFFF: 0x03}}
    for f16, by_r in want.items():
        q = torch.tensor([2 * step + f16 * step * 2.0 ** -16], dtype=torch.float64).float()      # exact in float32
        assert q.double().item() == 2 * step + f16 * step * 2.0 ** -16
        for r, code in by_r.items():
            assert _code(q.view(torch.int32).item(), r, fmt) == code, (hex(f16), hex(r))
    # fmax is a grid point: nothing passes it, and what the clamp brings there stays there; NaN is 0x7F whatever the draw
    top = {E4M3: 0x7E, E5M2: 0x7B}[fmt]
    x = torch.tensor([FMAX[fmt], float("inf"), 3e38, -float("inf"), float("nan"), -float("nan"), 0.0, -0.0])
    for r in (0, 0x8000, 0xFFFF):
        c = oo.codes_of(x, torch.ones(1), fmt, torch.full((8,), r)).tolist()
        assert c == [top, top, top, top | 0x80, 0x7F, 0x7F, 0x00, 0x80], r


@pytest.mark.parametrize("fmt", FMTS, ids=_ids)
def test_half_draws_give_the_rne_cast_except_on_exact_ties(fmt):
    """r = 0x8000 goes up exactly when the fraction is at least a half: round to nearest, ties away from zero"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(64, 257, generator=g) * torch.logspace(-7, 2, 64).view(-1, 1) * FMAX[fmt]
    grid = sro.grid(fmt)
    mids = (grid[:-1] + grid[1:]) / 2
    x[0, :mids.numel()] = mids
    x[1, :mids.numel()] = -mids
    x[2, :grid.numel()] = grid
    one = torch.ones(1)
    r = torch.full(x.shape, 0x8000)
    got = oo.codes_of(x, one, fmt, r)
    rne = oo.codes_of(x, one, fmt)
    q = torch.clamp(x, -FMAX[fmt], FMAX[fmt]).double()
    lo = oo.codes_of(x, one, fmt, torch.zeros_like(r)).view(fmt).double()
    hi = oo.codes_of(x, one, fmt, torch.full_like(r, 0xFFFF)).view(fmt).double()
    tie = (lo != hi) & ((q - lo) == (hi - q))
    assert tie.sum().item() >= 2 * mids.numel()
    assert torch.equal(got[~tie], rne[~tie])
    assert torch.equal(got[tie].view(fmt).double(), hi[tie])            # away from zero
    assert (got[tie] != rne[tie]).any() and (got[tie] == rne[tie]).any()   # RNE takes the even one: half of them differ


def test_the_three_oracles_agree_and_follow_the_flat_index():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(130, 136, generator=g)
    # one tile that covers the tensor is the per-tensor oracle under that tile's amax
    c0, s0, v0 = oo.oracle(x[:128, :128].contiguous(), x[:128, :128].abs().max().view(1), E5M2, seed=9)
    c1, s1, v1 = oo.oracle_block(x[:128, :128].contiguous(), E5M2, (128, 128), seed=9)
    assert torch.equal(oo.bits(c0), oo.bits(c1)) and s0.item() == s1.item() and torch.equal(v0, v1)
    # (128, 128): the transposed codes are the transposes; (1, 128): they are another quantization with the same draws
    cb, sb, _ = oo.oracle_block(x, E4M3, (128, 128), seed=4, offset=64)
    ct, st, _ = oo.oracle_block_t(x, E4M3, (128, 128), seed=4, offset=64)
    assert torch.equal(oo.bits(ct), oo.bits(cb).t()) and torch.equal(st, sb.t())
    # a row slice under its offset is the slice of the whole (row tiles: the scales are the rows' own)
    cw, _, _ = oo.oracle_block(x, E4M3, (1, 128), seed=4)
    cs, _, _ = oo.oracle_block(x[8:40].contiguous(), E4M3, (1, 128), seed=4, offset=8 * 136)
    assert torch.equal(oo.bits(cs), oo.bits(cw)[8:40])
    # without a seed the oracles are the round-to-nearest-even ones of tests/ocpb_oracle.py
    import ocpb_oracle as ob
    for tile in ob.TILES:
        a, b = oo.oracle_block(x, E4M3, tile), ob.oracle(x, E4M3, tile)
        assert all(torch.equal(oo.bits(p), oo.bits(q)) for p, q in zip(a, b))
    assert not torch.equal(oo.bits(cw), oo.bits(oo.oracle_block(x, E4M3, (1, 128), seed=5)[0]))


# ---- the header, the ctypes table, the library ----
def _decl(text, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_exactly_the_twelve_entries_and_keeps_the_version():
    text = open(os.path.join(ROOT, "include", "fp8q.h")).read()
    assert sorted(set(re.findall(r"^int (fp8q_ocp\w*sr_\w+)\(", text, re.M))) == ENTRIES and len(ENTRIES) == 12
    for name in ENTRIES:
        args = _decl(text, name)
        assert args[-3:] == ["uint64_t seed", "uint64_t offset", "fp8q_stream_t stream"], name
        assert args[:-3] + args[-1:] == _decl(text, TWINS[name[:-4]] + name[-4:]), name
    assert re.search(r"^#define FP8Q_VERSION 601\b", text, re.M)
    import fp8q
    assert fp8q.lib().fp8q_version() == 601


def test_lib_prototypes_match_the_header_and_the_draw_has_one_copy():
    import fp8q
    from fp8q import _lib, build
    for name in ENTRIES:
        res, args = _lib.SIGNATURES[name]
        tres, targs = _lib.SIGNATURES[TWINS[name[:-4]] + name[-4:]]
        assert res is ctypes.c_int and args == targs[:-1] + [ctypes.c_uint64, ctypes.c_uint64] + targs[-1:], name
        assert hasattr(fp8q.lib(), name)
    assert sorted(k for k in _lib.SIGNATURES if re.match(r"fp8q_ocp\w*sr_", k)) == ENTRIES
    # Philox, the draws and SR are the MX lane's: no OCP file defines them again
    for src in ("fp8q_ocpq.h", "fp8q_ocp.hip", "fp8q_ocp_block.hip", "fp8q_ocp_block_t.hip"):
        code = open(os.path.join(build.CSRC, src)).read()
        for fn in ("philox4x32(", "mx_sr(", "mx_draw8(", "mx_draw4(", "mx_draw1("):
            assert not re.search(r"^__device__ __forceinline__ \w+ %s" % re.escape(fn), code, re.M), (src, fn)
    assert '#include "fp8q_mxq.h"' in open(os.path.join(build.CSRC, "fp8q_ocpq.h")).read()


def test_c_abi_argument_errors_come_before_any_launch():
    import fp8q
    L = fp8q.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 63) & ~63             # never dereferenced: every call below is refused by the checks
    enc, ench, qnt, qnth = L.fp8q_ocpsr_encode_f32, L.fp8q_ocpsr_encode_h16, L.fp8q_ocpsr_quantize_f32, L.fp8q_ocpsr_quantize_h16
    benc, bench = L.fp8q_ocpbsr_encode_f32, L.fp8q_ocpbsr_encode_h16
    bqnt, bqnth = L.fp8q_ocpbsr_quantize_f32, L.fp8q_ocpbsr_quantize_h16
    tenc, tench = L.fp8q_ocpbtsr_encode_f32, L.fp8q_ocpbtsr_encode_h16
    both, bothh = L.fp8q_ocpbtsr_encode_both_f32, L.fp8q_ocpbtsr_encode_both_h16
    eps = 1e-8

    def every(off, seed=5, fmt=0, tile=(1, 128), R=4, K=128, x=p, half=BF16):
        tr, tk = tile
        return [enc(x, p, R, K, p, 1, fmt, eps, p, seed, off, None),
                ench(x, p, half, R, K, p, 1, fmt, eps, None, seed, off, None),
                qnt(x, p, R, K, p, R, fmt, eps, seed, off, None),
                qnth(x, p, half, half, R, K, p, 1, fmt, eps, seed, off, None),
                benc(x, p, p, R, K, tr, tk, fmt, eps, seed, off, None),
                bench(x, p, p, half, R, K, tr, tk, fmt, eps, seed, off, None),
                bqnt(x, p, R, K, tr, tk, fmt, eps, seed, off, None),
                bqnth(x, p, half, half, R, K, tr, tk, fmt, eps, seed, off, None),
                tenc(x, p, p, R, K, tr, tk, fmt, eps, seed, off, None),
                tench(x, p, p, half, R, K, tr, tk, fmt, eps, seed, off, None),
                both(x, p, p, p, p, R, K, tr, tk, fmt, eps, seed, off, None),
                bothh(x, p, p, p, p, half, R, K, tr, tk, fmt, eps, seed, off, None)]

    # an offset that is no multiple of 8, everything else in order
    for off in (1, 4, 7, 12, 2 ** 64 - 1, 2 ** 63 + 4):
        assert every(off) == [-1] * 12, off
        assert every(off, tile=(128, 128), fmt=1, half=F16) == [-1] * 12, off
    # the twin's refusals, with its codes: null pointers, formats, tiles, types, shapes, alignment
    assert every(0, x=None) == [-1] * 12
    for bad in (2, -1):
        assert every(0, fmt=bad) == [-2] * 12
    assert every(0, tile=(128, 1))[8:] == [-2] * 4 and every(8, tile=(2, 128))[4:] == [-2] * 8
    assert every(0, R=0) == [-1] * 12 and every(0, K=-1) == [-1] * 12
    assert every(0, x=p + 2)[0::2] == [-1] * 6                          # a float32 pointer off its 4 bytes
    assert every(0, x=p + 1)[1::2] == [-1] * 6                          # a half pointer off its 2
    assert every(0, half=F32)[1::2] == [-1] * 6
    assert qnth(p, p, F16, BF16, 4, 128, p, 1, 0, eps, 5, 0, None) == -1
    assert bqnth(p, p, F16, BF16, 4, 128, 1, 128, 0, eps, 5, 0, None) == -1
    assert enc(p, p, 4, 128, p, 3, 0, eps, p, 5, 0, None) == -1         # n_maxval not in {1, C}
    assert enc(p, None, 4, 128, p, 1, 0, eps, p, 5, 0, None) == -1 and enc(p, p, 4, 128, None, 1, 0, eps, p, 5, 0, None) == -1
    assert benc(p, p, None, 4, 128, 1, 128, 0, eps, 5, 0, None) == -1 and tenc(p, None, p, 4, 128, 1, 128, 0, eps, 5, 0, None) == -1
    for i in range(5):
        a = [p] * 5
        a[i] = None
        assert both(*a, 4, 128, 1, 128, 0, eps, 5, 0, None) == -1 and bothh(*a, F16, 4, 128, 1, 128, 0, eps, 5, 0, None) == -1


# ---- Python: the keywords ----
def _call(op):
    from fp8q import ops
    fn = getattr(ops, op)
    x = torch.randn(128, 128)
    if op in ("ocp_encode", "ocp_quantize"):
        return lambda **kw: fn(x, torch.ones(1), E4M3, **kw)
    return lambda **kw: fn(x, E4M3, **kw)


OPS = ("ocp_encode", "ocp_quantize", "ocp_block_encode", "ocp_block_quantize", "ocp_block_encode_t", "ocp_block_encode_both")


@pytest.mark.parametrize("op", OPS)
def test_seed_and_offset_refusals_arrive_before_the_device_check(op):
    from fp8q import ops
    call = _call(op)
    for bad in (True, False, 1.0, -1, 2 ** 64, torch.tensor(3), "7", (1,)):
        with pytest.raises(ops.Fp8qError, match="seed"):
            call(seed=bad)
    for bad in (True, 8.0, -8, 2 ** 64, torch.tensor(8), "8"):
        with pytest.raises(ops.Fp8qError, match="offset"):
            call(seed=1, offset=bad)
    for bad in (1, 4, 12, 2 ** 64 - 1):
        with pytest.raises(ops.Fp8qError, match="multiple of 8"):
            call(seed=1, offset=bad)
    with pytest.raises(ops.Fp8qError, match="without a seed"):
        call(offset=8)
    # keyword-only: no positional slot reaches them
    import inspect
    params = inspect.signature(getattr(ops, op)).parameters
    assert params["seed"].kind is inspect.Parameter.KEYWORD_ONLY and params["seed"].default is None
    assert params["offset"].kind is inspect.Parameter.KEYWORD_ONLY and params["offset"].default == 0
    # well-formed calls get as far as the device check
    for kw in (dict(seed=0), dict(seed=2 ** 64 - 1, offset=2 ** 64 - 8), dict(seed=None), dict(seed=None, offset=0)):
        with pytest.raises(ops.Fp8qError, match="CUDA"):
            call(**kw)


# ---- the quantizers ----
def test_quantizer_arguments_and_repr():
    from fp8q import ops
    from quantization.ocp import OCPBlockFP8Quantizer, OCPFP8Quantizer
    for cls in (OCPFP8Quantizer, OCPBlockFP8Quantizer):
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="stochastic"):
                cls(stochastic=bad)
        for bad in (True, 1.0, -1, 2 ** 64, None, torch.tensor(1)):
            with pytest.raises(ValueError, match="seed"):
                cls(stochastic=True, seed=bad)
            with pytest.raises(ValueError, match="seed"):
                cls(seed=bad)
        q = cls(fmt=E5M2)
        assert q.stochastic is False and q.seed == 0 and q.calls == 0 and q.last_seed is None
        assert "stochastic" not in q.extra_repr() and "seed" not in q.extra_repr()
        s = cls(fmt=E5M2, stochastic=True, seed=77)
        assert s.extra_repr() == q.extra_repr() + ", stochastic=True, seed=77"
        # the forward-only rule stays, and a refused call draws nothing
        with pytest.raises(NotImplementedError):
            s(torch.randn(32, 128, requires_grad=True))
        assert s.calls == 0
    assert OCPFP8Quantizer(fmt=E5M2).extra_repr().endswith("fmt=E5M2, eps=1e-08")
    assert OCPBlockFP8Quantizer(fmt=E5M2).extra_repr().endswith("fmt=E5M2, tile=1x128, eps=1e-08, flatten_rows=False")
    with pytest.raises(ops.Fp8qError, match="CUDA"):
        OCPBlockFP8Quantizer(stochastic=True)(torch.randn(32, 128))


def test_quantizer_bookkeeping(monkeypatch):
    from fp8q import ops
    from quantization.ocp import OCPBlockFP8Quantizer, OCPFP8Quantizer
    seen = []

    def fake(name):
        def op(x, *args, **kw):
            seen.append((name, kw.get("seed", "none")))
            return (x,) * 4 if "both" in name else ((x, x) if "encode" in name else x)
        return op

    for name in OPS:
        monkeypatch.setattr(ops, name, fake(name))
    x = torch.randn(128, 128)
    q = OCPBlockFP8Quantizer(stochastic=True, seed=2 ** 64 - 2)
    assert q.last_seed is None
    q(x)
    assert q.last_seed == 2 ** 64 - 2 and q.calls == 1
    q.encode(x)
    assert q.last_seed == 2 ** 64 - 1 and q.calls == 2
    q.encode_t(x)
    assert q.last_seed == 0 and q.calls == 3                   # mod 2^64
    q.encode_both(x)
    assert seen == [("ocp_block_quantize", 2 ** 64 - 2), ("ocp_block_encode", 2 ** 64 - 1), ("ocp_block_encode_t", 0),
                    ("ocp_block_encode_both", 1)]
    q.reseed(10)
    assert q.seed == 10 and q.calls == 0 and q.last_seed is None
    q(x)
    assert seen[-1] == ("ocp_block_quantize", 10) and q.last_seed == 10
    with pytest.raises(ValueError, match="seed"):
        q.reseed(-1)
    del seen[:]
    t = OCPFP8Quantizer(stochastic=True, seed=5)
    t.set_quant_range(torch.tensor(-1.0), torch.tensor(2.0))
    t(x)
    t.encode(x)
    assert seen == [("ocp_quantize", 5), ("ocp_encode", 6)] and t.last_seed == 6
    # not stochastic: the ops are called as they always were, without the keyword, and nothing is counted
    del seen[:]
    d, e = OCPFP8Quantizer(seed=3), OCPBlockFP8Quantizer(seed=3, tile=(128, 128))
    d.set_quant_range(torch.tensor(-1.0), torch.tensor(2.0))
    d(x), d.encode(x), e(x), e.encode(x), e.encode_t(x), e.encode_both(x)
    assert [s for _, s in seen] == ["none"] * 6 and d.calls == 0 and e.calls == 0 and e.last_seed is None


# ---- the frequency of rounding away from zero, on the oracle alone ----
@pytest.mark.parametrize("name", list(FREQ))
def test_frequency_on_the_oracle(name):
    fmt = FREQ[name][0]
    x = freq_input(name)
    ups = []
    for seed in FREQ_SEEDS:
        c, s, v = oo.oracle(x, torch.tensor([FMAX[fmt]]), fmt, seed=seed)
        assert s.item() == 1.0
        ups.append(freq_check(v.flatten(), name, f"{name} seed {seed}"))
    assert not torch.equal(ups[0], ups[1])
