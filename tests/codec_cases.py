"""Shared builders of the storage-code kernels' tests (tests/test_codec_routes_host.py, tests/test_codec_routes_gpu.py): the shapes
with the kernel each must reach, and the inputs.  A helper, not a test module; numpy only (and the host-only route query), needs no
GPU.  Formats, ranges, edge values and ties are those of tests/epilogue_cases.py, the input builder is
rows_cases.case_input(shape, fmt, "quantize"): every row has its own range out of ranges(fmt) -- neighbouring rows differ by orders
of magnitude, the degenerate ranges have rows of their own -- and the edge values of that range lie over the first and last
elements of every row, at every phase of a 16-byte group, and on both sides of every 4096-element chunk border.

  shapes    SHAPES: (encode, C, inner, fmt, fp_phase, code_phase, per_channel) -> the fields of ops.codec_route the case must find.
            fp_phase: the float32 side's offset from a 16-byte boundary in ELEMENTS (0..3), code_phase: the codes' in BYTES (0..15).
            Hand-written: each kernel's smallest shape and the lengths on both sides of each threshold; the format-dependent
            "tables fit" limit is found with the query and pinned as None -> whatever the query answers.
  variants  the completeness list: every (direction, kernel, variant) some shape must reach.
  all_codes every valid code of a format in every row.
"""
import numpy as np

import rows_cases as rc
from epilogue_cases import cycle, edge_values, fmt_me

E5M2, E4M3, E7 = rc.E5M2, rc.E4M3, rc.E7
FORMATS = [(2, 8, 1), (3, 8, 1), (5, 8, 1), (6, 8, 1), (3, 8, 0), (1, 8, 0), (2.5, 8, 1), (2, 4, 1), (3, 6, 0), (1, 3, 1)]
SLAB = 65535                # rows per launch of k_codec_rows
BIG = 1 << 20               # cases above this many elements run one format and are few


def _k(enc, C, inner, fmt=E5M2, fp=0, cp=0, pc=True):
    return (bool(enc), C, inner, fmt, fp, cp, pc)


def route_of(ops, key):
    enc, C, inner, fmt, fp, cp, pc = key
    return ops.codec_route(enc, C, inner, pc, *fmt, fp_mod16=4 * fp, code_mod16=cp)


def op_of(key):
    return "quantize" if key[6] else "quantize_pt"


def case_input(key):
    """rows_cases.case_input of the key's shape and format: per channel a range per row, per tensor the format's default range"""
    return rc.case_input((key[1], key[2]), key[3], op_of(key))


def variant(key, r):
    """the instances a route stands for, as the completeness list names them (a case can stand for several)"""
    enc, C, inner, fmt, fp, cp, pc = key
    if r["kernel"] == "k_rows_flat":
        out = ["nch>1" if r["nch"] > 1 else "nch=1"]
        if enc:
            out.append("wide" if r["wide"] else "!wide")
        return out
    if not pc:
        # what the kernel derives from the one row's addresses: stated by the case's phases, asserted by nothing but the result
        vec = fp == 0 and cp % 4 == 0
        out = ["pt_vec16" if vec and cp == 0 else ("pt_vec" if vec else "pt_scalar")]
    else:
        out = ["per_channel"]
    if r["launches"] > 1:
        out.append("launches>1")
    if r["steps"] > 1:
        out.append("steps>1")
    return out


def variants():
    """every (encode, kernel, variant) the shapes must reach between them"""
    V = set()
    for enc in (True, False):
        V |= {(enc, "k_rows_flat", v) for v in ("nch=1", "nch>1")}
        V |= {(enc, "k_codec_rows", v) for v in ("pt_vec16", "pt_vec", "pt_scalar", "per_channel", "launches>1", "steps>1")}
    V |= {(True, "k_rows_flat", "wide"), (True, "k_rows_flat", "!wide")}
    return V


STEPS2 = (1025, 4096 + 43)  # one block per row (2048 / 1025 rows), two pieces: the second step holds 2 (encode) / 10 (decode) groups and a tail


def _hand():
    S = {}
    flat, rows = "k_rows_flat", "k_codec_rows"
    for enc in (True, False):
        w = dict(wide=True) if enc else {}
        # ---- k_rows_flat
        S[_k(enc, 120, 147)] = dict(kernel=flat, nch=1, grid_x=5, **w)
        for fmt in FORMATS:                                               # (E4M3 among them)
            S.setdefault(_k(enc, 120, 147, fmt), dict(kernel=flat, nch=1, **w))
        for fmt in ((5, 8, 1), (2.5, 8, 1), E7):
            S[_k(enc, 9, 2048, fmt)] = dict(kernel=rows, grid_y=9)
        S[_k(enc, 29, 147)] = dict(kernel=flat, nch=1, grid_x=2, **w)      # 2nd chunk ragged (167 elements: lane 10 holds one group), tail 3
        S[_k(enc, 900, 7, (6, 8, 1))] = dict(kernel=flat, **w)            # the shortest rows any format's tables allow: b = 1, 2, 3 in turn
        S[_k(enc, 300, 37)] = dict(kernel=flat, **w)
        S[_k(enc, 300, 38)] = dict(kernel=flat, **w)
        S[_k(enc, 3, 2047)] = dict(kernel=flat, **w)
        S[_k(enc, 300, 40, (2, 4, 1))] = dict(kernel=flat, **w)
        S[_k(enc, 300, 41, (3, 6, 0))] = dict(kernel=flat, **w)
        S[_k(enc, 500, 9, (1, 3, 1))] = dict(kernel=flat, **w)
        for cp in (4, 8, 12):                                             # codes 4-byte but not 16-byte aligned; fp32 side aligned
            S[_k(enc, 120, 147, cp=cp)] = dict(kernel=flat, nch=1, wide=False)
        S[_k(enc, 57200, 147, E4M3)] = dict(kernel=flat, nch=2, **w)
        # ---- k_codec_rows, per tensor
        for n in (5, 16, 4096 + 7, 3 * 4096 + 21):
            S[_k(enc, 1, n, pc=False)] = dict(kernel=rows, grid_y=1, launches=1)
        S[_k(enc, 1, 3 * 4096 + 21, E4M3, pc=False)] = dict(kernel=rows, grid_x=4, steps=1)
        for fp, cp in ((0, 4), (0, 1), (1, 0), (3, 7)):
            S[_k(enc, 1, 4096 + 7, fp=fp, cp=cp, pc=False)] = dict(kernel=rows, grid_x=2)
        # ---- k_codec_rows, per channel
        S[_k(enc, 9, 2048)] = dict(kernel=rows, grid_y=9, grid_x=1)
        S[_k(enc, 17, 2049)] = dict(kernel=rows, grid_y=17)               # rows at every fp32 phase and code phases 0..15, row 16 at both zeros
        S[_k(enc, 3, 4099)] = dict(kernel=rows, grid_x=2)
        for inner in (1, 2, 3, 4, 5, 6):                                  # shorter than a group; 4..6: no format's tables fit next to a chunk
            S[_k(enc, 300, inner)] = dict(kernel=rows, grid_y=300)
        S[_k(enc, 900, 6, (6, 8, 1))] = dict(kernel=rows)
        for fp in (1, 2, 3):
            S[_k(enc, 120, 147, fp=fp)] = dict(kernel=rows)
        S[_k(enc, 120, 147, cp=1)] = dict(kernel=rows)
        S[_k(enc, 300, 40, E7)] = dict(kernel=rows)                       # 129-entry tables do not fit
        S[_k(enc, SLAB + 9, 3)] = dict(kernel=rows, launches=2, grid_y=SLAB)
        S[_k(enc, 70000, 5, fp=1)] = dict(kernel=rows, launches=2, grid_y=SLAB)
        S[_k(enc, *STEPS2)] = dict(kernel=rows, steps=2, grid_x=1, launches=1)
    return S


def flat_min_inner(ops, fmt, enc=True):
    """the shortest row k_rows_flat takes for the format (aligned pointers), by the query"""
    for i in range(4, 400):
        if route_of(ops, _k(enc, 300, i, fmt))["kernel"] == "k_rows_flat":
            return i
    raise AssertionError("no flat row below 400 for %r" % (fmt,))


def build_shapes(ops):
    """SHAPES for the library at hand: the hand-written expectations and, for the keys whose expectation is None, the query's
    own answer (the row lengths next to the format-dependent "tables fit" limit)"""
    S = _hand()
    for enc in (True, False):
        for fmt in (E7, (3, 8, 0), (2, 4, 1)):
            i = flat_min_inner(ops, fmt, enc)
            S.setdefault(_k(enc, 300, i, fmt), None)
            S.setdefault(_k(enc, 300, i - 1, fmt), None)
    for key in [k for k, v in S.items() if v is None]:
        r = route_of(ops, key)
        S[key] = dict(kernel=r["kernel"], nch=r["nch"], wide=r["wide"])
    return S


def all_codes(fmt, C, k=3):
    """[C, 2^n_bits * k] uint8: every row holds every valid code 0 .. 2^n_bits - 1 (k times), rotated by the row index.  With
    k = 3 no row length divides 4096: rows cross the chunk borders.  Codes with bits at or above n_bits are not defined
    (include/fp8q.h) and never appear."""
    n = 1 << fmt[1]
    return ((np.arange(n * k, dtype=np.int64)[None, :] + np.arange(C, dtype=np.int64)[:, None]) % n).astype(np.uint8)


def code_fields(codes, fmt):
    """(sign, exponent field, fraction field) of storage codes [sign | E | M]"""
    M, _ = fmt_me(fmt)
    mbits, n_bits, sign_bits = fmt
    c = codes.astype(np.int64)
    sign = (c >> (n_bits - 1)) & 1 if sign_bits else np.zeros_like(c)
    mag = c & ((1 << (n_bits - sign_bits)) - 1)
    return sign, mag >> M, mag & ((1 << M) - 1)


def n_edges(fmt):
    return len(edge_values(fmt[0], 1.0, fmt[2], fmt[1]))


def default_rows(case):
    """the rows whose range is the format's default one (integer bias: exact ties)"""
    rr = case["ranges"]
    return np.array([r for r, v in enumerate(rr) if v == rr[0]], np.int64)


def is_rich(key, case):
    """the rows of the default range hold the whole edge list between them"""
    sel = np.isin(case["pos"] // key[2], default_rows(case))
    return np.unique(case["idx"][sel]).size == n_edges(key[3])
