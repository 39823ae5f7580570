"""The multi-tensor launches of csrc/fp8q_multi.hip, rule by rule and branch by branch.  Every test first ASSERTS through
ops.multi_route (fp8q_multi_route: the launch's own plan builder, nothing enqueued) which launch each tensor lands in and whether
that is the batched k_multi_flat or the tensor's own single-tensor launch -- written out as literals, so that a changed rule
is noticed -- and then compares every output bit for bit (NaN matches NaN) with the CPU oracle: oracle.c_quantize (mode 0,
fp8q_multi_quantize_f32), c_encode (mode 3, fp8q_multi_encode_u8), c_decode (mode 4, fp8q_multi_decode_u8), c_minmax + c_absmax
(k_multi_rowmax behind fp8q_multi_minmax_quantize_f32 / _encode_u8).  Never with another call of the library.

Every tensor of a launch has its own scale of data and ranges and, where the case allows, its own format; the probes
0, -0, maxval, -maxval, 3 maxval, 1e-41, inf, -inf lie over its first elements and one NaN sits in one tensor of each
launch (tests/multi_cases.py).  Outputs are views into buffers pre-filled with a sentinel: what lies around a view must
still hold it afterwards.

  a  test_rule_*        each fall-back rule of plan_build at its boundary, the step structure
  b  test_flat_*        inside k_multi_flat<0 / 3 / 4>, every tensor asserted batched
  c  test_rowmax_*      k_multi_rowmax: loop edges, where the extreme sits, special rows
  d  test_refusal_*     a bad descriptor anywhere: an error, and nothing enqueued
"""
import ctypes

import numpy as np
import pytest
import torch

import multi_cases as mc
import oracle
from multi_cases import T

pytestmark = pytest.mark.gpu

FSENT, BSENT = -7.5, 0xA5          # what output buffers hold before a launch (neither is a value any case produces everywhere)
B, F, EMPTY = 1, 0, (-1, -1)       # fp8q_multi_route: batched / own launch / no launch


@pytest.fixture(scope="module")
def ops():
    import fp8q
    fp8q.lib()  # raises if libfp8q_hip.so is missing: no fallback
    return fp8q.ops


# ---------------------------------------------------------------------------------------------------------------------------
# device buffers at a chosen misalignment, with sentinel-filled slack around them
# ---------------------------------------------------------------------------------------------------------------------------
def _view(base, off_elems, shape):
    n = int(np.prod(shape, dtype=np.int64))
    assert base.data_ptr() % 16 == 0
    return base[off_elems:off_elems + n].view(tuple(shape))


def fdev(a, off=0):
    """float32 array on the device, `off` bytes (a multiple of 4) past a 16-byte boundary"""
    a = np.ascontiguousarray(a, np.float32)
    v = _view(torch.zeros(a.size + 8, dtype=torch.float32, device="cuda"), off // 4, a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def bdev(a, off=0):
    a = np.ascontiguousarray(a, np.uint8)
    v = _view(torch.zeros(a.size + 32, dtype=torch.uint8, device="cuda"), off, a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def fout(shape, off=0):
    n = int(np.prod(shape, dtype=np.int64))
    base = torch.full((n + 8,), FSENT, dtype=torch.float32, device="cuda")
    return _view(base, off // 4, shape), base


def bout(shape, off=0):
    n = int(np.prod(shape, dtype=np.int64))
    base = torch.full((n + 32,), BSENT, dtype=torch.uint8, device="cuda")
    return _view(base, off, shape), base


def slack_untouched(base, view):
    sent = BSENT if base.dtype == torch.uint8 else FSENT
    o = (view.data_ptr() - base.data_ptr()) // base.element_size()
    return bool((base[:o] == sent).all()) and bool((base[o + view.numel():] == sent).all())


def same_bits(got, ref, what):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if ref.dtype == np.uint8:
        bad = got != ref
    else:
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern, first at " \
            f"{np.argwhere(np.isnan(got) != np.isnan(ref))[:4].tolist()}"
        bad = (got.view(np.int32) != ref.view(np.int32)) & ~np.isnan(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {ref.size} elements differ, first at {np.argwhere(bad)[:4].tolist()}: " \
        f"got {got[bad][:4].tolist()}, expected {ref[bad][:4].tolist()}"


def descs_of(items):
    """fp8q_tensor_desc array of (x, maxval, mbits, n_bits, sign_bits, out) items, by hand: dim 0 is the channel when maxval
    has more than one element"""
    import fp8q
    d = (fp8q._lib.TensorDesc * len(items))()
    for e, (x, mv, M, nb, sb, out) in zip(d, items):
        assert x.is_contiguous() and mv.is_contiguous() and out.is_contiguous()
        C = x.shape[0] if mv.numel() != 1 else 1
        e.x, e.y, e.maxval = x.data_ptr(), out.data_ptr(), mv.data_ptr()
        e.C, e.inner, e.n_maxval = C, (x.numel() // C if C else 0), mv.numel()
        e.mbits, e.n_bits, e.sign_bits = float(M), int(nb), int(sb)
    return d


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(ops, mode, items):
    """the entry point of a mode on (x, maxval, mbits, n_bits, sign_bits, out) items; outputs in item order"""
    if mode == 0:
        outs = ops.multi_quantize(items)
    elif mode == 4:
        outs = ops.multi_decode(items)
    else:   # encode with GIVEN ranges has no Python wrapper (ops.multi_minmax_encode finds them first: section c)
        import fp8q
        assert fp8q.lib().fp8q_multi_encode_u8(descs_of(items), len(items), stream()) == 0
        outs = [it[5] for it in items]
    assert len(outs) == len(items) and all(o.data_ptr() == it[5].data_ptr() for o, it in zip(outs, items)), "item order"
    return outs


def build(mode, specs, seed, nan_in=0, with_probes=True):
    """items, references and output buffers of one launch.  Mode 4 decodes the oracle's codes of the same data."""
    rng = np.random.RandomState(seed)
    items, refs, bases = [], [], []
    for i, s in enumerate(specs):
        x, mv = mc.make(s, i, rng, with_probes)
        if i == nan_in and x.size > 16:
            x.reshape(-1)[x.size // 2 + 1] = np.nan
        M, nb, sb = s.fmt
        if x.size == 0:
            src, ref = x, np.empty(x.shape, np.uint8 if mode == 3 else np.float32)
        elif mode == 0:
            src, ref = x, oracle.c_quantize(x, mv, M, nb, sb)
        elif mode == 3:
            src, ref = x, oracle.c_encode(x, mv, M, nb, sb)
        else:
            src = oracle.c_encode(x, mv, M, nb, sb)
            ref = oracle.c_decode(src, mv, M, nb, sb)
        xin = bdev(src, s.xoff) if mode == 4 else fdev(src, s.xoff)
        out, base = (bout if mode == 3 else fout)(s.shape, s.yoff)
        items.append((xin, fdev(mv), M, nb, sb, out))
        refs.append(ref)
        bases.append(base)
    return items, refs, bases


def run(ops, mode, specs, expect, seed, nan_in=0):
    items, refs, bases = build(mode, specs, seed, nan_in)
    assert ops.multi_route(items, mc.MODES[mode]) == expect, "route"
    outs = call(ops, mode, items)
    for i, (s, y, ref, base) in enumerate(zip(specs, outs, refs, bases)):
        same_bits(y, ref, f"mode {mode} tensor {i} {s}")
        assert slack_untouched(base, y), f"mode {mode} tensor {i} {s}: wrote outside its output"


# ---------------------------------------------------------------------------------------------------------------------------
# a. the batching rules at their boundaries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 3, 4])
@pytest.mark.parametrize("fmt,lo,hi,modes", mc.ROW_TABLE_EDGES, ids=lambda v: str(v).replace(" ", ""))
def test_rule_row_tables_fit_36k(ops, mode, fmt, lo, hi, modes):
    """rpc * per_row <= 36 KiB: per-channel [16, inner] falls back at `lo`, batches at `hi` = lo + 1"""
    if mode not in modes:
        import fp8q
        src = fdev(np.ones((16, hi))) if mode == 3 else bdev(np.zeros((16, hi)))
        item = (src, fdev(np.ones(16)), *fmt, (bout if mode == 3 else fout)((16, hi))[0])
        with pytest.raises(fp8q.Fp8qError, match="unsupported"):   # E = 0: no storage codes, the query refuses like the launch
            ops.multi_route([item], mc.MODES[mode])
        return
    run(ops, mode, [T((16, lo), fmt), T((16, hi), fmt)], [(0, F), (1, B)], seed=10 + mode)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_rule_magic_divisor_and_four_elements(ops, mode):
    """inner <= kMagicMaxDivisor = 60000; nelem >= 4 (a per-tensor [1, 3] has no 16-byte group)"""
    specs = [T((2, 60000), (3, 8, 1)), T((2, 60001), (2, 8, 1)), T((1, 3), (4, 8, 1), True), T((1, 4), (5, 8, 1), True)]
    run(ops, mode, specs, [(0, B), (1, F), (2, F), (3, B)], seed=20 + mode)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_rule_alignment(ops, mode):
    """16-byte groups of fp32 on the value side, 4-byte groups of codes on the other: each misalignment falls back on its own,
    its aligned twin (same shape, same format) batches"""
    shape = (24, 43)
    if mode == 0:
        off = [(4, 0), (0, 4)]
    elif mode == 3:
        off = [(4, 0), (0, 1), (0, 2), (0, 3)]
    else:
        off = [(1, 0), (2, 0), (3, 0), (0, 4)]
    specs, expect = [], []
    for k, (xo, yo) in enumerate(off):
        fmt = [(3, 8, 1), (2, 8, 1), (4, 8, 1), (5, 8, 1)][k]
        specs += [T(shape, fmt), T(shape, fmt, False, xo, yo)]
        expect += [(2 * k, B), (2 * k + 1, F)]
    # codes that are 4-byte but not 16-byte aligned still batch
    specs.append(T(shape, (3, 8, 1), False, 4 if mode == 4 else 0, 4 if mode == 3 else 0))
    expect.append((2 * len(off), B))
    run(ops, mode, specs, expect, seed=30 + mode)


def test_rule_64_mib(ops):
    """nelem * 4 < 64 MiB, mode 0: [4096, 4096] is exactly 64 MiB and takes its own (nontemporal) launch, [4096, 4095] is
    batched -- 4096 chunks of one tensor.  Four bands of 64 rows against the oracle, the whole against ops.quantize, which
    tests/test_large_regime.py ties to the oracle."""
    g = torch.Generator(device="cuda").manual_seed(41)
    items, hosts = [], []
    for i, (shape, M) in enumerate([((4096, 4096), 3), ((4096, 4095), 2)]):
        s = float(mc.scale_of(3 + 4 * i))
        x = torch.randn(shape, generator=g, device="cuda") * s
        mv = (torch.rand(shape[0], generator=g, device="cuda") * 2 + 0.6) * s
        x.view(-1)[:8] = torch.from_numpy(mc.probes(mv[0].item())).cuda()
        x[2049 - i, 77] = float("nan")
        items.append((x, mv, M, 8, 1, torch.full(shape, FSENT, device="cuda")))
    assert ops.multi_route(items, "quantize") == [(0, F), (1, B)], "route"
    outs = ops.multi_quantize(items)
    for (x, mv, M, _, _, _), y in zip(items, outs):
        for lo in (0, 2016, 3000, 4096 - 64):
            ref = oracle.c_quantize(x[lo:lo + 64].cpu().numpy(), mv[lo:lo + 64].cpu().numpy(), M, 8, 1)
            same_bits(y[lo:lo + 64], ref, f"{tuple(x.shape)} rows {lo}..{lo + 64}")
        whole = ops.quantize(x, mv, M, 8, 1)
        assert torch.equal(torch.isnan(y), torch.isnan(whole))
        assert torch.equal(y.nan_to_num(1.0).view(torch.int32), whole.nan_to_num(1.0).view(torch.int32)), tuple(x.shape)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_rule_step_structure(ops, mode):
    """32 tensors per batched launch; a fall-back closes the batch before it and gets a step of its own, in order; empty tensors
    get none; outputs stay in item order"""
    fmts = [(3, 8, 1), (2, 8, 1), (4, 8, 1), (5, 8, 1)]
    specs = [T((3 + i % 5, 40 + i), fmts[i % 4]) for i in range(33)]
    run(ops, mode, specs, [(0, B)] * 32 + [(1, B)], seed=50 + mode, nan_in=32)
    specs = [T((16, 40), fmts[0]), T((0, 9), fmts[1]), T((9, 44), fmts[1]), T((16, 5), fmts[2]), T((5, 0, 3), fmts[0]),
             T((7, 47), fmts[3])]
    run(ops, mode, specs, [(0, B), EMPTY, (0, B), (1, F), EMPTY, (2, B)], seed=53 + mode)


# ---------------------------------------------------------------------------------------------------------------------------
# b. inside k_multi_flat: every tensor asserted batched
# ---------------------------------------------------------------------------------------------------------------------------
def rows_for(inner, elems):
    return -(-elems // inner) + 1


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_flat_rows_shorter_than_two_groups(ops, mode):
    """the in-group row boundary (b < 4) at every phase of a 16-byte group, several boundaries per lane: inner 6, 7, 9, 11 at
    (7,8,1) (mode 0: no codes without an exponent bit) and 7, 9, 11 at (6,8,1), three chunks each, hundreds of table rows"""
    specs = [T((rows_for(i, 8200 + 4096 * (i % 2)), i), (6, 8, 1)) for i in (7, 9, 11)]
    if mode == 0:
        specs += [T((rows_for(i, 8200), i), (7, 8, 1)) for i in (6, 7, 9, 11)]
    run(ops, mode, specs, [(0, B)] * len(specs), seed=60 + mode, nan_in=1)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_flat_rows_at_every_group_phase(ops, mode):
    """inner 34 .. 37 at (2,8,1) -- 33-entry tables, ~120 rows per chunk -- and 4099, a row longer than a chunk"""
    specs = [T((rows_for(i, 8200), i), (2, 8, 1)) for i in (34, 35, 36, 37)] + [T((3, 4099), (3, 8, 1))]
    run(ops, mode, specs, [(0, B)] * 5, seed=63 + mode, nan_in=4)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_flat_chunk_edges_32_tensors(ops, mode):
    """4096 k + t and 4096 k + 4 + t elements (k = 1, 2; t = 0 .. 3): the last chunk is exactly full and owns the tail
    (rem <= kChunkElems), or holds one group plus the tail.  Per tensor and per channel: 32 tensors, one launch, descriptor 31
    in use."""
    fmts = [(3, 8, 1), (2, 8, 1), (4, 8, 1), (5, 8, 1), (2, 6, 1)]
    specs = [T((C * n,), fmts[k % 5], True) for k, (C, n) in enumerate(mc.CHUNK_EDGE_SHAPES)]
    specs += [T((C, n), fmts[(k + 2) % 5], C == 1) for k, (C, n) in enumerate(mc.CHUNK_EDGE_SHAPES)]
    run(ops, mode, specs, [(0, B)] * 32, seed=66 + mode, nan_in=31)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_flat_mixed_table_layouts(ops, mode):
    """(1,8,0) at inner 125: 129-entry tables, 34 rows; (6,8,1) at inner 7: 3-entry tables, 587 rows; a per-tensor entry: every
    tensor's tables sit behind chl + rpc_max of the LAUNCH, not of the tensor"""
    specs = [T((70, 125), (1, 8, 0)), T((1300, 7), (6, 8, 1)), T((5003,), (3, 8, 1), True), T((41, 125), (1, 8, 0)),
             T((90, 57), (4, 8, 1))]
    run(ops, mode, specs, [(0, B)] * 5, seed=70 + mode, nan_in=3)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_flat_32_single_chunk_tensors(ops, mode):
    """32 tensors of one chunk each: chunk g belongs to descriptor g, up to descriptor 31"""
    fmts = [(3, 8, 1), (2, 8, 1), (4, 8, 1), (5, 8, 1), (3, 8, 0), (2, 6, 1)]
    specs = [T((3000 + 31 * i,), fmts[i % 6], True) if i % 4 == 1 else T((8 + i, 40 + 2 * i), fmts[i % 6]) for i in range(32)]
    assert all(int(np.prod(s.shape)) <= 4096 for s in specs)
    run(ops, mode, specs, [(0, B)] * 32, seed=73 + mode, nan_in=31)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_flat_formats_below_8_bits_and_unsigned(ops, mode):
    """n_bits 6, 4, 5 (the codes' sign bit sits at n_bits - 1) and sign_bits = 0 with negative inputs, which clamp to 0"""
    specs = []
    for k, fmt in enumerate([(2, 6, 1), (1, 4, 0), (3, 5, 1), (3, 8, 0), (1, 8, 0), (2, 6, 0)]):
        specs += [T((rows_for(131 + k, 4300), 131 + k), fmt), T((4200 + 5 * k + k % 4,), fmt, True)]
    run(ops, mode, specs, [(0, B)] * 12, seed=76 + mode, nan_in=5)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_flat_more_chunks_than_blocks(ops, mode):
    """~1300 chunks over 32 tensors of different formats (5 M elements): more than the 1024 blocks of the launch, so blocks
    stride from one tensor's chunk to another's with different tables"""
    fmts = [(3, 8, 1), (2, 8, 1), (4, 8, 1), (5, 8, 1), (6, 8, 1), (3, 8, 0), (2, 6, 1), (7, 8, 1) if mode == 0 else (3, 5, 1)]
    specs = [T((163841 + 4099 * i,), fmts[i % 8], True) if i % 5 == 2 else T((60 + i, 2500 + 37 * i), fmts[i % 8])
             for i in range(32)]
    assert sum(-(-int(np.prod(s.shape)) // 4096) for s in specs) > 1024
    run(ops, mode, specs, [(0, B)] * 32, seed=80 + mode, nan_in=17)


def test_flat_decode_of_encode_is_quantize(ops):
    """decode(encode(x)) == quantize(x) through the multi-tensor entry points, for the formats and ranges at which
    tests/test_codes.py establishes that identity: codes against c_encode, decoded values against c_quantize"""
    rng = np.random.RandomState(90)
    enc, xs = [], []
    for k, (M, sb, mv) in enumerate(mc.ROUNDTRIP_FORMATS):
        for shape in [(5000 + 3 * k,), (40 + k, 131)]:
            x = (rng.standard_normal(shape) * mv / 2.2).astype(np.float32)
            x.reshape(-1)[:8] = mc.probes(mv)
            rng_shape = 1 if len(shape) == 1 else shape[0]
            xs.append((x, np.full(rng_shape, mv, np.float32), M, sb))
            enc.append((fdev(x), fdev(xs[-1][1]), M, 8, sb, bout(shape)[0]))
    assert ops.multi_route(enc, "encode") == [(0, B)] * 16, "route"
    codes = call(ops, 3, enc)
    dec = [(c, it[1], it[2], 8, it[4], fout(c.shape)[0]) for c, it in zip(codes, enc)]
    assert ops.multi_route(dec, "decode") == [(0, B)] * 16, "route"
    ys = call(ops, 4, dec)
    for (x, mv, M, sb), c, y in zip(xs, codes, ys):
        same_bits(c, oracle.c_encode(x, mv, M, 8, sb), f"codes {x.shape} M={M} sign={sb}")
        same_bits(y, oracle.c_quantize(x, mv, M, 8, sb), f"round trip {x.shape} M={M} sign={sb}")


# ---------------------------------------------------------------------------------------------------------------------------
# c. k_multi_rowmax through multi_minmax_quantize / multi_minmax_encode
# ---------------------------------------------------------------------------------------------------------------------------
ROWMAX_INNERS = [4, 63, 64, 65, 192, 193, 255, 256, 257, 449, 16385]
# the quantize / encode launch behind the ranges: inner 4 is too short for per-row tables at any format (own launch, step 0),
# the ten others share step 1; then the 4-byte-aligned view (own launch)
ROWMAX_ROUTES = [(0, F)] + [(1, B)] * 10 + [(2, F)]
ROWMAX_FMTS = [(3, 8, 1), (2, 8, 1), (4, 8, 1), (5, 8, 1)]


def rowmax_tensor(inner, i, rng):
    """[12, inner]: one row per place the extreme can sit and per kind of special row (see the comments)"""
    s = mc.scale_of(i)
    x = (rng.standard_normal((12, inner)) * s).astype(np.float32)
    pos = mc.rowmax_positions(inner)
    main = pos["main"] if pos["main"] is not None else inner // 2
    rem = pos["rem"] if pos["rem"] is not None else inner // 2
    big = np.float32(40) * s
    x[0, 0] = big                           # the maximum in the first element
    x[1, inner - 1] = -big                  # the minimum, larger in magnitude than the maximum, in the last element
    x[2, main] = -big                       # the extreme read by the loop with four loads in flight ...
    x[3, rem] = big                         # ... and by the one-load remainder loop
    x[4] = -np.abs(x[4]) - s                # all negative: max < 0, maxval = |min|
    x[5] = -0.0                             # only -0.0: range 0, the channel quantizes to NaN (the reference's quirk)
    x[6, main] = np.inf
    x[7, rem] = -np.inf
    x[8] = (rng.randint(1, 1 << 22, inner).astype(np.uint32) | (np.arange(inner, dtype=np.uint32) % 2) << 31) \
        .view(np.float32)                   # denormals of both signs
    x[9, main] = np.nan                     # a NaN read by the four-deep loop ...
    x[10, rem] = np.nan                     # ... and by the remainder loop
    return x


def check_ranges(got_mv, x, what):
    mn, mx = oracle.c_minmax(x, True)
    mv = oracle.c_absmax(mn, mx)
    same_bits(got_mv, mv, what + " ranges")
    return mv


@pytest.mark.parametrize("entry", ["quantize", "encode"])
def test_rowmax_loop_edges_and_special_rows(ops, entry):
    """inner at each edge of `i + 192 < inner` and of the 64-lane remainder; ranges against c_minmax + c_absmax, then values /
    codes against the oracle on those ranges"""
    rng = np.random.RandomState(100)
    xs = [rowmax_tensor(inner, i, rng) for i, inner in enumerate(ROWMAX_INNERS)]
    for inner, x in zip(ROWMAX_INNERS, xs):      # the rows do reach both loops wherever the row length has both
        kinds = {mc.rowmax_loop(p, inner) for p in range(inner)}
        assert kinds == ({"rem"} if inner <= 192 else {"main"} if inner == 256 else {"main", "rem"}), inner
    xs.append(rowmax_tensor(449, 11, rng))       # the view that is only 4-byte aligned
    items, bases = [], []
    for i, x in enumerate(xs):
        out, base = (fout if entry == "quantize" else bout)(x.shape)
        mv_out, mv_base = fout((x.shape[0],))
        M, nb, sb = ROWMAX_FMTS[i % 4]
        items.append((fdev(x, 4 if i == len(xs) - 1 else 0), mv_out, M, nb, sb, out))
        bases.append((base, mv_base))
    assert ops.multi_route(items, entry) == ROWMAX_ROUTES, "route"
    outs = (ops.multi_minmax_quantize if entry == "quantize" else ops.multi_minmax_encode)(items)
    for i, (x, it, y, (base, mv_base)) in enumerate(zip(xs, items, outs, bases)):
        what = f"{entry} tensor {i} {x.shape}"
        mv = check_ranges(it[1], x, what)
        ref = (oracle.c_quantize if entry == "quantize" else oracle.c_encode)(x, mv, it[2], it[3], it[4])
        same_bits(y, ref, what)
        assert slack_untouched(base, y) and slack_untouched(mv_base, it[1]), what


@pytest.mark.parametrize("entry", ["quantize", "encode"])
def test_rowmax_40_tensors_of_differing_rows(ops, entry):
    """rows of all tensors are numbered consecutively and looked up by ballot over row0: 40 tensors of 1 .. 79 rows, two range
    launches (32 + 8), two batched quantize / encode launches"""
    rng = np.random.RandomState(110)
    items, xs = [], []
    for i in range(40):
        shape = (1 + (i * 7) % 79, 40 + 5 * i)
        x = (rng.standard_normal(shape) * mc.scale_of(i)).astype(np.float32)
        x[shape[0] // 2, (i * 13) % shape[1]] *= 30
        if i == 33:
            x[0, 3] = np.nan
        xs.append(x)
        M, nb, sb = ROWMAX_FMTS[i % 4]
        items.append((fdev(x), fout((shape[0],))[0], M, nb, sb, (fout if entry == "quantize" else bout)(shape)[0]))
    assert ops.multi_route(items, entry) == [(0, B)] * 32 + [(1, B)] * 8, "route"
    outs = (ops.multi_minmax_quantize if entry == "quantize" else ops.multi_minmax_encode)(items)
    for i, (x, it, y) in enumerate(zip(xs, items, outs)):
        mv = check_ranges(it[1], x, f"{entry} tensor {i}")
        ref = (oracle.c_quantize if entry == "quantize" else oracle.c_encode)(x, mv, it[2], it[3], it[4])
        same_bits(y, ref, f"{entry} tensor {i} {x.shape}")


# ---------------------------------------------------------------------------------------------------------------------------
# d. a bad descriptor anywhere: an error, and nothing enqueued
# ---------------------------------------------------------------------------------------------------------------------------
def refusal_items(codes):
    rng = np.random.RandomState(120)
    items, bases = [], []
    for i, shape in enumerate([(16, 40), (9, 4099), (16, 5), (30, 125)]):     # batched, batched, own launch, batched
        out, base = (bout if codes else fout)(shape)
        mv, mv_base = fout((shape[0],))
        items.append((fdev(rng.standard_normal(shape) * mc.scale_of(i)), mv, 3, 8, 1, out))
        bases += [base, mv_base]
    return items, bases


def all_sentinel(bases):
    torch.cuda.synchronize()
    return all(bool((b == (BSENT if b.dtype == torch.uint8 else FSENT)).all()) for b in bases)


def test_refusal_quantize_wrong_range_length_last(ops):
    """fp8q_multi_quantize_f32: three good descriptors, then one whose n_maxval is neither 1 nor C"""
    import fp8q
    items, bases = refusal_items(False)
    for it in items:
        it[1].fill_(1.0)                                  # (input ranges here; the outputs keep their sentinel)
    bases = bases[0::2]
    assert ops.multi_route(items, "quantize") == [(0, B), (0, B), (1, F), (2, B)], "route"
    bad = items[:3] + [(items[3][0], items[3][1][:3], 3, 8, 1, items[3][5])]
    with pytest.raises(fp8q.Fp8qError):
        ops.multi_quantize(bad)
    with pytest.raises(fp8q.Fp8qError):
        ops.multi_route(bad, "quantize")
    d = descs_of(items)
    d[3].n_maxval = 3                                     # the C entry point itself, behind the wrapper's own check
    assert fp8q.lib().fp8q_multi_quantize_f32(d, 4, stream()) == -1
    assert all_sentinel(bases)
    assert fp8q.lib().fp8q_multi_quantize_f32(descs_of(items), 4, stream()) == 0       # the good list does run
    assert not all_sentinel(bases)


def test_refusal_minmax_encode_no_exponent_bit_last(ops):
    """fp8q_multi_minmax_encode_u8: the last item is (7,8,1), E = 0 -- refused before the range launch, which would have
    overwritten every maxval_out"""
    import fp8q
    items, bases = refusal_items(True)
    bad = items[:3] + [items[3][:2] + (7, 8, 1) + items[3][5:]]
    with pytest.raises(fp8q.Fp8qError, match="unsupported"):
        ops.multi_minmax_encode(bad)
    assert all_sentinel(bases)
    assert ops.multi_route(items, "encode") == [(0, B), (0, B), (1, F), (2, B)], "route"
    ops.multi_minmax_encode(items)
    assert not all_sentinel(bases)


def test_refusal_minmax_quantize_foreign_range_buffer(ops):
    """fp8q_multi_minmax_quantize_f32: descs[i].maxval must be NULL or maxval_out[i]; a range buffer elsewhere would be
    ignored, so it is refused -- by hand, the Python wrapper cannot build such a descriptor"""
    import fp8q
    items, bases = refusal_items(False)
    d = descs_of(items)
    mv_out = (ctypes.c_void_p * 4)(*[it[1].data_ptr() for it in items])
    elsewhere = torch.ones(30, device="cuda")
    d[3].maxval = elsewhere.data_ptr()
    assert fp8q.lib().fp8q_multi_minmax_quantize_f32(d, mv_out, 4, stream()) == -1
    assert all_sentinel(bases)
    d[3].maxval = None                                    # NULL is the other permitted value
    assert fp8q.lib().fp8q_multi_minmax_quantize_f32(d, mv_out, 4, stream()) == 0
    for it in items:
        x = it[0].cpu().numpy()
        same_bits(it[5], oracle.c_quantize(x, check_ranges(it[1], x, "after the refusal"), 3, 8, 1), "after the refusal")
