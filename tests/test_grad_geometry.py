"""Every branch of the backward kernels' shared launch plan (csrc/fp8q_bwd.h: bwd_plan), FP family (csrc/fp8q_grad.hip).

The shape lists of test_grad_kernels.py leave whole branches of k_bwd_rows / k_bwd_short / k_bwd_final unrun: a block that
takes a second, strided piece of its row, per-channel rows split over several blocks, three of the seven lane-group widths
of the short-row kernel, every boundary between two widths, and a block that moves on to a second group of rows.  This
file runs them, by the criteria of test_grad_kernels.py and with its checker (_check): gx bit-identical to the torch chain,
gmaxval / gmbits within 2^-22 of the float64 host sum of the same fp32 terms relative to sum |term| (per row), the "grad"
workspace all zero after every call.

Which branch a shape takes is decided here by a Python restatement of bwd_plan() and balanced_blocks() whose constants are
READ from the sources (a changed constant fails test_plan_constants_and_coverage instead of quietly moving a shape into
another branch).  Every GPU test asserts, through that mirror, the class it is named for before it launches.

Classes (labels of `classes()`):
  short rows    "short G=<1..64>", and "short <lut|direct> <one pass|several passes>" (lut: the row tables of the FP
                kernel in LDS, taken when inner >= 2 * (pmax + 1); several passes: a block walks more than one group of rows)
  long rows     "long <tensor|channel> U=<1|4> <cached|nt> <single|strided> nsplit<=1|>1>"
                strided: the block cap binds, a block streams the pieces s, s + nsplit, ... of its row (base += step is taken
                with a full piece behind it); single: one planned piece per block
                "long ragged extra trip": the row's last, partial piece is not among the planned ones, so the first splits
                go round the loop once more for it (a full trip, then a ragged one, in the same block)
The nontemporal long-row loop cannot be strided below 64 Mi elements (its cap is kBwdMaxItems pieces of 4096 elements): out
of scope, and asserted unreachable by the table.  Its body is the template instantiated for the cached, strided cases.
"""
import collections
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_grad_kernels import FORMATS, _bits, _check, _data, _workspace_is_zero

gpu = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fp8-quantization_amd", "csrc")

# what the shapes below were worked out for
EXPECTED_CONSTANTS = dict(kShortMaxInner=2048, kBwdMaxItems=16384, g_elems=24, g_max=64, small_limit=8 << 20, kTargetBlocks=2048,
                          kUnroll=4, kBlock=256, nt_bytes=64 << 20)


def _one(text, pattern, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, f"{what}: expected exactly one match of {pattern!r} in the sources, found {len(found)}"
    return found[0]


@functools.lru_cache(maxsize=None)
def plan_constants():
    """the constants of bwd_plan(), read from csrc/ (each pattern also pins the line of the rule it stands in)"""
    def src(name):
        with open(os.path.join(CSRC, name)) as fh:
            return fh.read()
    bwd, common, device, grad = src("fp8q_bwd.h"), src("fp8q_common.h"), src("fp8q_device.h"), src("fp8q_grad.hip")
    k = {}
    k["kShortMaxInner"] = int(_one(bwd, r"constexpr int kShortMaxInner = (\d+);", "kShortMaxInner"))
    k["kBwdMaxItems"] = int(_one(bwd, r"constexpr int64_t kBwdMaxItems = (\d+);", "kBwdMaxItems"))
    g_max, g_elems = _one(bwd, r"while \(G < (\d+) && \(int64_t\)G \* (\d+) < inner\) G <<= 1;", "the lanes-per-row rule")
    k["g_max"], k["g_elems"] = int(g_max), int(g_elems)
    a, b = _one(bwd, r"const bool small = C == 1 && inner < \(\(int64_t\)(\d+) << (\d+)\);", "the small-tensor limit")
    k["small_limit"] = int(a) << int(b)
    k["kTargetBlocks"] = int(_one(common, r"constexpr int kTargetBlocks = (\d+);", "kTargetBlocks"))
    k["kUnroll"] = int(_one(common, r"constexpr int kUnroll = (\d+);", "kUnroll"))
    k["kBlock"] = int(_one(device, r"constexpr int kBlock = (\d+);", "kBlock"))
    a, b = _one(common, r"return \(int64_t\)\(v >= 1 \? v : (\d+)\) << (\d+);", "the default of kNtBytes")
    k["nt_bytes"] = int(a) << int(b)
    # the rest of the plan, line by line: a rewritten rule must come back to this mirror
    for text, line in [
        (bwd, "p.nt = C * inner * 4 >= kNtBytes;"),
        (bwd, "if (per_channel && inner <= kShortMaxInner) {"),
        (bwd, "p.blocks = balanced_blocks(cdiv(C, kBlock / G), kBwdMaxItems);"),
        (bwd, "if (small) p.U = 1;"),
        (bwd, "const int64_t pieces = inner / (4 * kBlock * p.U) > 0 ? inner / (4 * kBlock * p.U) : 1;"),
        (bwd, "const int64_t total_cap = p.nt ? kBwdMaxItems : kTargetBlocks;"),
        (bwd, "const int64_t cap = total_cap / C > 0 ? total_cap / C : 1;"),
        (bwd, "p.nsplit = balanced_blocks(pieces, cap);"),
        (common, "if (pieces <= cap) return pieces < 1 ? 1 : pieces;"),
        (common, "const int64_t steps = (pieces + cap - 1) / cap;"),
        (common, "return (pieces + steps - 1) / steps;"),
        (common, "f->pmax = 1 << E;"),
        (grad, "const bool lut = sums && p.inner >= 2 * (int64_t)bf.lut_stride;"),
    ]:
        assert text.count(line) == 1, f"the sources no longer hold the line {line!r} exactly once"
    assert grad.count("bf.lut_stride = bf.tab[0].pmax + 1;") == 2
    return k


def cdiv(a, b):
    return (a + b - 1) // b


def balanced_blocks(pieces, cap):
    cap = max(cap, 1)
    if pieces <= cap:
        return max(pieces, 1)
    steps = cdiv(pieces, cap)
    return cdiv(pieces, steps)


Plan = collections.namedtuple("Plan", "shortrows G C inner nsplit blocks U nt pieces trips")


def bwd_plan(C, inner, n_range):
    """bwd_plan() of csrc/fp8q_bwd.h; `pieces`: planned pieces (short rows: passes) in all, `trips`: the most times a
    block goes round its loop"""
    k = plan_constants()
    per_channel = n_range != 1
    if not per_channel:
        C, inner = 1, C * inner
    nt = C * inner * 4 >= k["nt_bytes"]
    U = k["kUnroll"]
    if per_channel and inner <= k["kShortMaxInner"]:
        G = 1
        while G < k["g_max"] and G * k["g_elems"] < inner:
            G <<= 1
        npass = cdiv(C, k["kBlock"] // G)
        blocks = balanced_blocks(npass, k["kBwdMaxItems"])
        return Plan(True, G, C, inner, 0, blocks, U, nt, npass, cdiv(npass, blocks))
    if C == 1 and inner < k["small_limit"]:
        U = 1
    pieces = max(inner // (4 * k["kBlock"] * U), 1)
    cap = max((k["kBwdMaxItems"] if nt else k["kTargetBlocks"]) // C, 1)
    nsplit = balanced_blocks(pieces, cap)
    trips = cdiv(cdiv(inner >> 2, k["kBlock"] * U), nsplit)            # of split 0: base = 0, step, 2 step, ... < nvec
    return Plan(False, 0, C, inner, nsplit, C * nsplit, U, nt, pieces, trips)


def pmax_of(n_bits, mbits, sign_bits):
    """make_fmt(): the largest table index of a format"""
    hi = n_bits - sign_bits
    M = min(max(int(np.rint(np.float32(mbits))), 1), hi)
    return 1 << (hi - M)


def classes(C, inner, per_channel, fmt=None, device_width=False):
    """the labels of the branches that a call with range gradients takes; fmt = (n_bits, mbits, sign_bits) for the FP
    family (whose short-row kernel has a table variant), None for the INT family"""
    p = bwd_plan(C, inner, C if per_channel else 1)
    if p.shortrows:
        lut = False
        if fmt is not None:
            stride = pmax_of(fmt[0], 1.0 if device_width else fmt[1], fmt[2]) + 1
            lut = p.inner >= 2 * stride
        return {f"short G={p.G}", f"short {'lut' if lut else 'direct'} {'one pass' if p.trips <= 1 else 'several passes'}"}
    strided = p.pieces > p.nsplit
    out = {f"long {'channel' if per_channel else 'tensor'} U={p.U} {'nt' if p.nt else 'cached'} "
           f"{'strided' if strided else 'single'} nsplit{'>1' if p.nsplit > 1 else '=1'}"}
    if not strided and p.trips > 1:
        out.add("long ragged extra trip")
    return out


def assert_classes(C, inner, per_channel, want, fmt=None, device_width=False):
    assert os.environ.get("FP8Q_NT_MB") is None, "the nontemporal threshold is a tuning knob: these tests run at its default"
    got = classes(C, inner, per_channel, fmt, device_width)
    assert got == set(want), f"[{C},{inner}] per_channel={per_channel} fmt={fmt}: the plan takes {sorted(got)}, the test is for {sorted(want)}"


# ------------------------------------------------------------------------------------------------------------------
# the shapes: name -> (C, inner, per_channel, classes without the short-row table label)
# ------------------------------------------------------------------------------------------------------------------
RAGGED = "long ragged extra trip"
LONG_SHAPES = {
    # per tensor, U = 1
    "tensor_u1_one_block": (1, 1027, False, {"long tensor U=1 cached single nsplit=1"}),
    "tensor_u1_single": (1, 4097, False, {"long tensor U=1 cached single nsplit>1"}),
    # 3072 pieces of 1024 elements over 1536 blocks: two full trips each, split 0 a third one for the last 5 elements
    "tensor_u1_strided": (1, 3 * (1 << 20) + 5, False, {"long tensor U=1 cached strided nsplit>1"}),
    # per tensor, U = 4, below 64 MiB
    "tensor_u4_single": (1, (1 << 23) + 5, False, {"long tensor U=4 cached single nsplit>1", RAGGED}),
    # 2049 pieces of 4096 elements over 1025 blocks
    "tensor_u4_strided": (1, 2049 * 4096 + 5, False, {"long tensor U=4 cached strided nsplit>1"}),
    # per tensor, 64 MiB: 4096 pieces, 4096 blocks, split 0 a second trip for the last 5 elements
    "tensor_nt": (1, (1 << 24) + 5, False, {"long tensor U=4 nt single nsplit>1", RAGGED}),
    # per channel, rows split over blocks: part_a per (row, split)
    "channel_split2": (3, 2 * 4096 + 5, True, {"long channel U=4 cached single nsplit>1", RAGGED}),
    "channel_split5": (3, 5 * 4096 + 1027, True, {"long channel U=4 cached single nsplit>1", RAGGED}),
    # per channel, the cap binds: 2048 / 1025 = 1 block per row, three trips, the last one ragged
    "channel_cap1": (1025, 2 * 4096 + 1029, True, {"long channel U=4 cached strided nsplit=1"}),
    # 2048 / 700 = 2 blocks per row over 5 planned pieces (and a ragged sixth): three trips per block
    "channel_cap2": (700, 5 * 4096 + 7, True, {"long channel U=4 cached strided nsplit>1"}),
    # per channel, 64 MiB: 1024 pieces per row, 16384 / 4 = 4096 blocks allowed
    "channel_nt": (4, (1 << 22) + 3, True, {"long channel U=4 nt single nsplit>1"}),
}
# what the plan must say about them beyond the class (the arithmetic of the comments above)
LONG_DETAILS = {
    "tensor_u1_strided": dict(pieces=3072, nsplit=1536, trips=3),
    "tensor_u4_single": dict(pieces=2048, nsplit=2048, trips=2),
    "tensor_u4_strided": dict(pieces=2049, nsplit=1025, trips=2),
    "tensor_nt": dict(pieces=4096, nsplit=4096, trips=2),
    "channel_split2": dict(pieces=2, nsplit=2, trips=2),
    "channel_split5": dict(pieces=5, nsplit=5, trips=2),
    "channel_cap1": dict(pieces=2, nsplit=1, trips=3),
    "channel_cap2": dict(pieces=5, nsplit=2, trips=3),
    "channel_nt": dict(pieces=1024, nsplit=1024, trips=1),
}
BIG = 8 << 20                     # from here on: one format, no cached data, device tensors freed

# short rows: C = 37 leaves dead row slots in the last block at every G; every boundary of the G rule, and 2049, the first
# row of the long-row kernel
SWEEP_C = 37
SWEEP = {24: 1, 25: 2, 48: 2, 49: 4, 96: 4, 97: 8, 192: 8, 193: 16, 384: 16, 385: 32, 768: 32, 769: 64, 2047: 64, 2048: 64,
         2049: None}
SWEEP_LONG = {"long channel U=4 cached single nsplit=1"}
# from which row length on a format's tables go to LDS in k_bwd_short: 2 * (pmax + 1), pmax = 2^(exponent bits)
LUT_FROM = {(8, 2.0, 1): 66, (8, 3.0, 1): 34, (8, 3.0, 0): 66, (6, 2.0, 1): 18, (8, 5.0, 0): 18}
assert list(LUT_FROM) == FORMATS

# short rows, several passes per block: 16385 passes of 256 rows (G = 1) and one of 44 over 8193 blocks, two each
LOOP_C = 16384 * 256 + 300
LOOP_INNER = 5
LOOP_CLASSES = {"short G=1", "short direct several passes"}
# ... with the tables: E0M7 (8 bits, 7 mantissa bits, signed) has the smallest pmax that make_fmt gives, 1, so rows of 4
LOOP_LUT_FMT = (8, 7.0, 1)
LOOP_LUT_INNER = 4
LOOP_LUT_CLASSES = {"short G=1", "short lut several passes"}

BIG_FMT = (8, 3.0, 1)

FULL = (
    {f"short G={G}" for G in (1, 2, 4, 8, 16, 32, 64)}
    | {"short lut one pass", "short direct one pass", "short lut several passes", "short direct several passes"}
    | {"long tensor U=1 cached single nsplit=1", "long tensor U=1 cached single nsplit>1", "long tensor U=1 cached strided nsplit>1",
       "long tensor U=4 cached single nsplit>1", "long tensor U=4 cached strided nsplit>1", "long tensor U=4 nt single nsplit>1",
       "long channel U=4 cached single nsplit=1", "long channel U=4 cached single nsplit>1",
       "long channel U=4 cached strided nsplit=1", "long channel U=4 cached strided nsplit>1",
       "long channel U=4 nt single nsplit>1", RAGGED})
OUT_OF_SCOPE = {"long tensor U=4 nt strided nsplit>1", "long channel U=4 nt strided nsplit>1", "long channel U=4 nt strided nsplit=1"}


def test_plan_constants_and_coverage():
    """no GPU: the constants are the ones the shapes were chosen for, every shape is in the class it is listed under, and
    the shapes of this file and of test_int_grad_geometry.py reach every class"""
    assert plan_constants() == EXPECTED_CONSTANTS
    assert os.environ.get("FP8Q_NT_MB") is None
    reached = set()
    for name, (C, inner, pc, want) in LONG_SHAPES.items():
        got = classes(C, inner, pc, BIG_FMT)
        assert got == want, f"{name}: {sorted(got)}"
        assert got == classes(C, inner, pc, None), name                   # the INT family: the same plan
        p = bwd_plan(C, inner, C if pc else 1)
        for key, val in LONG_DETAILS.get(name, {}).items():
            assert getattr(p, key) == val, f"{name}: {key} = {getattr(p, key)}, expected {val}"
        assert (C * inner * 4 >= 64 << 20) == ("nt" in next(iter(want - {RAGGED})).split()), name
        reached |= got
    for inner, G in SWEEP.items():
        for fmt in FORMATS:
            got = classes(SWEEP_C, inner, True, fmt)
            if G is None:
                assert got == SWEEP_LONG
            else:
                lut = inner >= LUT_FROM[fmt]
                assert got == {f"short G={G}", f"short {'lut' if lut else 'direct'} one pass"}, f"inner={inner} {fmt}: {sorted(got)}"
            reached |= got
        reached |= classes(SWEEP_C, inner, True, None)
    # G's boundaries sit where the rule says: 24 elements per lane
    for G, last in ((1, 24), (2, 48), (4, 96), (8, 192), (16, 384), (32, 768), (64, 2048)):
        assert bwd_plan(SWEEP_C, last, SWEEP_C).G == G
        assert last == 2048 or bwd_plan(SWEEP_C, last + 1, SWEEP_C).G == 2 * G
    got = classes(LOOP_C, LOOP_INNER, True, BIG_FMT)
    assert got == LOOP_CLASSES == classes(LOOP_C, LOOP_INNER, True, None)
    p = bwd_plan(LOOP_C, LOOP_INNER, LOOP_C)
    assert (p.pieces, p.blocks, p.trips, p.nt) == (16386, 8193, 2, True) and LOOP_C - 16385 * 256 == 44
    reached |= got
    got = classes(LOOP_C, LOOP_LUT_INNER, True, LOOP_LUT_FMT)
    assert got == LOOP_LUT_CLASSES
    assert pmax_of(*LOOP_LUT_FMT) == 1 == min(pmax_of(nb, mb, sb) for nb in range(2, 17) for sb in (0, 1)
                                              for mb in range(1, 17) if 0 <= nb - sb - min(mb, nb - sb) <= 7)
    # the smallest row that takes the tables, still on one lane
    assert LOOP_LUT_INNER == 2 * (pmax_of(*LOOP_LUT_FMT) + 1) <= 24
    reached |= got
    print("\n".join(sorted(reached)))
    assert reached == FULL, f"not reached: {sorted(FULL - reached)}; unexpected: {sorted(reached - FULL)}"
    assert not reached & OUT_OF_SCOPE


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _gx_only_matches(x, g, mv, fmt, full_gx, what):
    """SUMS = false: the call that wants gx alone, bit for bit the gx of the call with everything"""
    from fp8q import ops
    nb, mb, sb = fmt
    gx, gmv, gmb = ops.quantize_backward(x, g, mv, mb, nb, sb, True, False, False)
    assert gmv is None and gmb is None
    assert torch.equal(_bits(gx), _bits(full_gx)), f"{what}: gx of the call without sums differs"


def _device_width_matches(x, g, mv, fmt, full, what):
    """the width as a device scalar: the same three results to the bit"""
    from fp8q import ops
    nb, mb, sb = fmt
    dev = ops.quantize_backward(x, g, mv, torch.tensor([mb], device="cuda"), nb, sb, True, True, True)
    assert _workspace_is_zero(x), what
    for a, b, name in zip(dev, full, ("gx", "gmaxval", "gmbits")):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: {name} differs between host and device width"


def _run_long(name, monkeypatch, seed):
    C, inner, pc, want = LONG_SHAPES[name]
    big = C * inner >= BIG
    for k, fmt in enumerate([BIG_FMT] if big else FORMATS):
        assert_classes(C, inner, pc, want, fmt)
        nb, mb, sb = fmt
        x, g, mv = _data(C, inner, pc, seed + k)
        if not pc:
            x, g = x.view(-1), g.view(-1)
        what = f"{name} [{C},{inner}] fmt={fmt}"
        full = _check(x, g, mv, mb, nb, sb, pc, monkeypatch, what)
        if fmt == BIG_FMT:
            assert_classes(C, inner, pc, want, fmt, device_width=True)
            _device_width_matches(x, g, mv, fmt, full, what)
            if name == "tensor_u1_strided":
                _gx_only_matches(x, g, mv, fmt, full[0], what)
        del x, g, mv, full
        torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("name", ["channel_split2", "channel_split5"])
def test_per_channel_rows_split_over_blocks(name, monkeypatch):
    """every row against its own host sum: a row that picks up its neighbour's partials fails"""
    _run_long(name, monkeypatch, 700)


@gpu
@pytest.mark.parametrize("name", ["channel_cap1", "channel_cap2"])
def test_per_channel_rows_block_cap_binds(name, monkeypatch):
    _run_long(name, monkeypatch, 710)


@gpu
@pytest.mark.parametrize("name", ["tensor_u1_one_block", "tensor_u1_single", "tensor_u1_strided", "tensor_u4_single", "tensor_u4_strided"])
def test_per_tensor(name, monkeypatch):
    """(the 64 MiB per-tensor shape of the table, tensor_nt, is test_grad_kernels.py::test_per_tensor_rows[16777221])"""
    _run_long(name, monkeypatch, 720)


@gpu
def test_per_channel_nontemporal_split(monkeypatch):
    _run_long("channel_nt", monkeypatch, 730)


@gpu
@pytest.mark.parametrize("inner", list(SWEEP))
def test_short_rows_every_group_width_and_boundary(inner, monkeypatch):
    G = SWEEP[inner]
    for k, fmt in enumerate(FORMATS):
        nb, mb, sb = fmt
        if G is None:
            want = SWEEP_LONG
        else:
            want = {f"short G={G}", f"short {'lut' if inner >= LUT_FROM[fmt] else 'direct'} one pass"}
        assert_classes(SWEEP_C, inner, True, want, fmt)
        x, g, mv = _data(SWEEP_C, inner, True, 740 + k)
        _check(x, g, mv, mb, nb, sb, True, monkeypatch, f"short rows [{SWEEP_C},{inner}] fmt={fmt}")


@gpu
def test_short_rows_several_passes(monkeypatch):
    """[4194604, 5]: G = 1, no tables, 8193 blocks of two passes each, the last pass with 44 live rows of 256"""
    assert_classes(LOOP_C, LOOP_INNER, True, LOOP_CLASSES, BIG_FMT)
    nb, mb, sb = BIG_FMT
    x, g, mv = _data(LOOP_C, LOOP_INNER, True, 750)
    what = f"short rows, two passes [{LOOP_C},{LOOP_INNER}]"
    full = _check(x, g, mv, mb, nb, sb, True, monkeypatch, what)
    assert_classes(LOOP_C, LOOP_INNER, True, LOOP_CLASSES, BIG_FMT, device_width=True)
    _device_width_matches(x, g, mv, BIG_FMT, full, what)
    _gx_only_matches(x, g, mv, BIG_FMT, full[0], what)
    del x, g, mv, full
    torch.cuda.empty_cache()


@gpu
def test_short_rows_several_passes_with_tables(monkeypatch):
    """Format (n_bits, mbits, sign_bits) = (8, 7.0, 1): no exponent bits, pmax = 1, the smallest make_fmt gives; the tables
    go to LDS from rows of 2 * (pmax + 1) = 4 elements, and rows of 4 are still on one lane (G = 1).  [4194604, 4] =
    16778416 elements: 8193 blocks rebuild the 256 row tables of their second pass between two barriers, and part_b adds up
    over both passes.  Every row is checked."""
    assert_classes(LOOP_C, LOOP_LUT_INNER, True, LOOP_LUT_CLASSES, LOOP_LUT_FMT)
    nb, mb, sb = LOOP_LUT_FMT
    x, g, mv = _data(LOOP_C, LOOP_LUT_INNER, True, 760)
    full = _check(x, g, mv, mb, nb, sb, True, monkeypatch, f"short rows with tables, two passes [{LOOP_C},{LOOP_LUT_INNER}]")
    del x, g, mv, full
    torch.cuda.empty_cache()
