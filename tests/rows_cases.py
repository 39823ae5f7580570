"""Shared builders of the row kernels' tests (tests/test_rows_routes_host.py, tests/test_rows_routes_gpu.py): the shapes with the
kernel each must reach, and the input tensors that carry the hand-picked hard values of tests/epilogue_cases.py to every row
border and chunk border.  A helper, not a test module; numpy only (and the host-only route query), needs no GPU.

  shapes    SHAPES: (op, C, inner, fmt, x_phase, y_phase, in_place) -> the fields of ops.rows_route the case must find
            (kernel and the launcher-chosen variant).  op is one of ops.ROWS_OPS; "quantize_pt" / "minmax_pt" are their per-tensor
            calls ([C, inner] seen as one row).  x_phase / y_phase: the first element's offset from a 16-byte boundary, in
            elements.  The hand-written part names each kernel's smallest shape and the lengths on both sides of every
            threshold; the swept part (k_rows_reg's (lanes, slots) pairs, the staged kernels' groups, the format-dependent
            "tables fit" / "staged window fits" limits) is found with the route query itself and pinned by VARIANTS: the
            completeness list every (op, kernel, variant) of which some shape must reach.
  inputs    case_input: see there.  Every row has its own range; the edge values of that range lie over the first and the last
            elements of the row (epilogue_cases.edge_slots: at every phase of a 16-byte group over the rows) and on both sides
            of every 4096-element chunk border.
"""
import numpy as np

from epilogue_cases import edge_index, edge_slots, edge_values, is_plain, ranges, ties

E5M2, E4M3, E7 = (2, 8, 1), (3, 8, 1), (1, 8, 0)
NARROW = (7, 8, 1)          # no exponent bit: two table entries, the smallest tables
CHUNK = 4096
BORDER = 8                  # edge values on each side of a chunk border
SMALL_ELEMS = 16384         # k_small_rows_fused: C * inner up to here


def pc_of(op):
    return not op.endswith("_pt")


def base_op(op):
    return op[:-3] if op.endswith("_pt") else op


def route_of(ops, key):
    op, C, inner, fmt, xp, yp, ip = key
    return ops.rows_route(base_op(op), C, inner, pc_of(op), *fmt, x_mod16=4 * xp, y_mod16=4 * yp, in_place=ip)


def variant(key, r):
    """the launcher-chosen instance a route stands for, as the completeness list names it"""
    op, k = key[0], r["kernel"]
    if k == "k_rows_flat":
        if op != "quantize":
            return "fused"
        return "nch>1" if r["nch"] > 1 else "nch=1"
    if k == "k_rows_direct":
        return "minmax" if op == "minmax" else ("lut" if r["lut"] else "nolut")
    if k == "k_quant_rows":
        return "per_channel" if pc_of(op) else ("small" if r["small"] else "big")
    if k == "k_small_rows_fused":
        return "epl%d" % r["slots"]
    if k == "k_rows_reg":
        return "phase%d" % key[4] if op == "minmax" else "L%dx%d" % (r["lanes"], r["slots"])
    if k in ("k_rows_staged", "k_rows_staged_mm"):
        return "group%d" % r["group"]
    if k == "k_minmax_partial":
        return ("nsplit=1" if r["nsplit"] == 1 else "nsplit>1") + ("" if pc_of(op) else "_pt")
    return ""


# the (lanes, slots) instances k_rows_reg's selection rule can pick for fused rows: pinned here, found again by reg_sweep
REG_PAIRS = ([(16, e) for e in range(2, 9)] + [(32, e) for e in range(5, 9)] + [(64, e) for e in range(5, 9)] +
             [(256, e) for e in range(3, 9)])
REG_ROWS = 16               # rows of the long-row fused shapes: one of every row kind of fused_kinds


def reg_sweep(ops):
    """(lanes, slots) -> the shortest row that reaches it: the route query asked for every multiple of 4 in 128..8192"""
    out = {}
    for inner in range(128, 8193, 4):
        r = ops.rows_route("minmax_quantize", _rows_for(inner), inner, True, *E4M3)
        if r["kernel"] == "k_rows_reg":
            out.setdefault((r["lanes"], r["slots"]), inner)
    return out


def _rows_for(inner, above=True):
    """a handful of rows with C * inner on the far side of the small-tensor limit"""
    return max(REG_ROWS, SMALL_ELEMS // inner + 1) if above else max(1, min(5, SMALL_ELEMS // inner))


def _k(op, C, inner, fmt=E5M2, xp=0, yp=None, ip=False):
    return (op, C, inner, fmt, xp, xp if (yp is None or ip) else yp, ip)


def _hand():
    q, f, m = "quantize", "minmax_quantize", "minmax"
    S = {}
    # ---- K1
    S[_k(q, 120, 147)] = dict(kernel="k_rows_flat", nch=1, group=8)
    S[_k(q, 120, 147, ip=True)] = dict(kernel="k_rows_flat", nch=1)
    S[_k(q, 57200, 147, E4M3)] = dict(kernel="k_rows_flat", nch=2, grid_x=1024)       # > 2 * 1023 chunks: two per tile, resident grid
    S[_k(q, 3, 2047)] = dict(kernel="k_rows_flat", group=64)
    S[_k(q, 9, 2048)] = dict(kernel="k_quant_rows", small=False, grid_y=9)
    S[_k(q, 3, 2049, xp=1)] = dict(kernel="k_quant_rows", grid_y=3)                   # rows peel to their own alignment
    S[_k(q, 3, 2049, xp=1, yp=2)] = dict(kernel="k_quant_scalar", grid_y=3)
    S[_k(q + "_pt", 7, 1001, E4M3)] = dict(kernel="k_quant_rows", small=True, grid_y=1)
    S[_k(q + "_pt", 3, 555, E4M3, xp=3)] = dict(kernel="k_quant_rows", small=True)
    S[_k(q + "_pt", 3, 555, E4M3, xp=3, yp=0)] = dict(kernel="k_quant_scalar", grid_y=1)
    S[_k(q + "_pt", 2048, 4096 + 1, E4M3)] = dict(kernel="k_quant_rows", small=False, nontemporal=False, grid_x=2048)   # >= 8 Mi elements
    for inner, fmt in ((3, E5M2), (4, E5M2), (40, E5M2), (65, E5M2), (66, E5M2), (31, E4M3), (32, E4M3), (33, E4M3)):
        S[_k(q, 300, inner, fmt)] = None      # rows on both sides of 2 * (pmax + 1) and of 4: whatever the query says (below)
    for xp in (1, 2, 3):                      # pointers 4, 8 and 12 bytes off: co-aligned and not
        S[_k(q, 120, 147, xp=xp)] = dict(kernel="k_rows_direct", lut=True)
        S[_k(q, 120, 147, xp=xp, yp=0)] = dict(kernel="k_rows_direct", lut=True)
        S[_k(q, 200, 40, xp=xp, ip=True)] = dict(kernel="k_rows_direct", lut=False)
    # ---- fused
    for C, inner, epl in ((7, 5, 1), (1, 64, 1), (100, 65, 2), (100, 128, 2), (100, 129, 3), (60, 200, 4), (63, 256, 4), (50, 257, 8),
                          (32, 512, 8), (3, 3, 1), (4096, 4, 1)):
        S[_k(f, C, inner)] = dict(kernel="k_small_rows_fused", slots=epl)
    S[_k(f, 7, 5, ip=True)] = dict(kernel="k_small_rows_fused", slots=1)
    S[_k(f, 50, 257, E4M3, xp=1, yp=3)] = dict(kernel="k_small_rows_fused", slots=8)
    S[_k(f, 120, 147)] = dict(kernel="k_rows_staged", group=8, nch=1)
    S[_k(f, 120, 147, E7)] = dict(kernel="k_rows_flat", nch=1)                        # 129-entry tables: the window does not fit
    S[_k(f, 300, 64)] = dict(kernel="k_rows_flat", nch=1)                             # 66 rows of tables per chunk: neither
    S[_k(f, 120, 147, ip=True)] = dict(kernel="k_rows_direct", lut=True)
    S[_k(f, 120, 147, xp=2)] = dict(kernel="k_rows_direct", lut=True)
    S[_k(f, REG_ROWS, 8193)] = dict(kernel="k_rows_direct", lut=True, group=64)
    S[_k(f, REG_ROWS, 16384, E4M3)] = dict(kernel="k_rows_direct", lut=True)
    S[_k(f, 70, 259)] = dict(kernel="k_rows_direct", lut=True)
    S[_k(f, 70, 257, E7)] = dict(kernel="k_rows_direct", lut=False)                   # rows above 256, shorter than 2 * 129
    S[_k(f, 300, 64, E7, ip=True)] = dict(kernel="k_rows_direct", lut=False)
    S[_k(f, 4100, 4)] = dict(kernel="k_rows_direct", lut=False)
    S[_k(f, 5500, 3)] = dict(kernel="k_rows_direct", lut=False)
    S[_k(f, 33, 513)] = dict(kernel="k_rows_direct", lut=True)
    S[_k(f, 33, 512)] = dict(kernel="k_rows_reg", lanes=16, slots=8)
    S[_k(f, 33, 512, ip=True)] = dict(kernel="k_rows_reg", lanes=16, slots=8)
    S[_k(f, REG_ROWS, 8192)] = dict(kernel="k_rows_reg", lanes=256, slots=8)
    S[_k(f, 65, 256)] = dict(kernel="k_rows_reg", lanes=16, slots=4)
    # the thresholds by launcher.  fp8q_minmax_quantize_f32: 16384 elements and rows of 512 (k_small_rows_fused); fp8q_launch_rows_reg
    # with quant: rows of 128 .. 8192, a multiple of 4; launch_rows_flat fused: rows of 4 .. 256 (3/4 and 256/257 above).  67/68
    # is the min/max side of fp8q_launch_rows_reg only, 2047/2048 fp8q_direct_max_inner (K1 and min/max only): both further down.
    S[_k(f, 130, 127)] = dict(kernel="k_rows_staged", group=4)
    S[_k(f, 129, 128)] = dict(kernel="k_rows_reg", lanes=16, slots=2)
    S[_k(f, 65, 257)] = dict(kernel="k_rows_direct", lut=True)
    S[_k(f, 245, 67)] = None
    S[_k(f, 241, 68)] = None
    # ---- min/max
    for xp in range(4):
        S[_k(m, 6, 514, xp=xp)] = dict(kernel="k_rows_reg", lanes=32, slots=5)        # rows at every 4-byte phase, two tail scalars
        S[_k(m, 7, 147, xp=xp)] = dict(kernel="k_rows_direct" if xp else "k_rows_staged_mm")
    S[_k(m, 5, 67)] = dict(kernel="k_rows_staged_mm", group=4)
    S[_k(m, 5, 68)] = dict(kernel="k_rows_staged_mm", group=4)
    S[_k(m, 5, 127)] = dict(kernel="k_rows_reg", lanes=16, slots=2)
    S[_k(m, 5, 128)] = dict(kernel="k_rows_reg", lanes=16, slots=2)
    S[_k(m, 70, 256)] = dict(kernel="k_rows_reg", lanes=16, slots=4)
    S[_k(m, 70, 257)] = dict(kernel="k_rows_reg", lanes=16, slots=5)
    S[_k(m, 300, 3)] = dict(kernel="k_rows_direct")
    S[_k(m, 300, 4)] = dict(kernel="k_rows_staged_mm", group=1)
    S[_k(m, 400, 40)] = dict(kernel="k_rows_staged_mm", group=2)
    S[_k(m, 120, 147)] = dict(kernel="k_rows_staged_mm", group=8)
    S[_k(m, 3, 2047)] = dict(kernel="k_rows_reg", lanes=64, slots=8)
    S[_k(m, 3, 2048)] = dict(kernel="k_rows_reg", lanes=64, slots=8)
    S[_k(m, 3, 8192)] = dict(kernel="k_rows_reg", lanes=256, slots=8)
    S[_k(m, 3, 8193)] = dict(kernel="k_minmax_partial", nsplit=2, grid_x=3, grid_y=3)
    S[_k(m, 2, 16384 + 5, xp=1)] = dict(kernel="k_minmax_partial", nsplit=3)
    S[_k(m, 5, 2052)] = dict(kernel="k_minmax_partial", nsplit=1, grid_x=1)           # rows k_rows_reg fills badly, too long for the rest
    S[_k(m + "_pt", 7, 1001)] = dict(kernel="k_minmax_partial", nsplit=1, grid_y=1)
    S[_k(m + "_pt", 3, 555, xp=3)] = dict(kernel="k_minmax_partial", nsplit=1)
    S[_k(m + "_pt", 9, 8193, xp=1)] = dict(kernel="k_minmax_partial", nsplit=10)
    return S


def build_shapes(ops):
    """SHAPES for the library at hand: the hand-written expectations, the swept ones, and for the keys whose expectation is
    None the query's own answer (the lengths next to a format-dependent limit: the test then compares whatever is reached)"""
    S = _hand()
    f, q = "minmax_quantize", "quantize"
    for (lanes, slots), inner in sorted(reg_sweep(ops).items()):
        S.setdefault(_k(f, _rows_for(inner), inner, E4M3), dict(kernel="k_rows_reg", lanes=lanes, slots=slots))
    for fmt in (E5M2, E4M3, NARROW, E7):
        # k_rows_staged: every group, and the shortest / longest row whose window + tables fit (the lengths next to them too)
        fits = [i for i in range(4, 257) if route_of(ops, _k(f, _rows_for(i), i, fmt))["kernel"] == "k_rows_staged"]
        seen = {}
        for i in fits:
            seen.setdefault(route_of(ops, _k(f, _rows_for(i), i, fmt))["group"], i)
        for g, i in seen.items():
            S.setdefault(_k(f, _rows_for(i), i, fmt), dict(kernel="k_rows_staged", group=g))
        for i in ([fits[0] - 1, fits[0], fits[-1]] if fits else []):
            if i >= 4:
                S.setdefault(_k(f, _rows_for(i), i, fmt), None)
        # K1: the shortest row whose tables fit k_rows_flat's LDS budget, and the one below it
        flat = [i for i in range(4, 400) if route_of(ops, _k(q, 300, i, fmt))["kernel"] == "k_rows_flat"]
        for i in ([flat[0] - 1, flat[0]] if flat else []):
            if i >= 4:
                S.setdefault(_k(q, 300, i, fmt), None)
    for key in [k for k, v in S.items() if v is None]:
        r = route_of(ops, key)
        S[key] = dict(kernel=r["kernel"], lut=r["lut"], nch=r["nch"], group=r["group"])
    # both sides of the small-tensor limit at one row length
    S.setdefault(_k(f, 64, 256), dict(kernel="k_small_rows_fused", slots=4))
    return S


def variants():
    """every (op, kernel, variant) the shapes must reach between them"""
    q, f, m = "quantize", "minmax_quantize", "minmax"
    V = {(q, "k_rows_flat", "nch=1"), (q, "k_rows_flat", "nch>1"),
         (q, "k_rows_direct", "lut"), (q, "k_rows_direct", "nolut"), (q, "k_quant_rows", "per_channel"),
         (q + "_pt", "k_quant_rows", "small"), (q + "_pt", "k_quant_rows", "big"), (q, "k_quant_scalar", ""),
         (q + "_pt", "k_quant_scalar", ""),
         (f, "k_rows_flat", "fused"), (f, "k_rows_direct", "lut"), (f, "k_rows_direct", "nolut"),
         (m, "k_rows_direct", "minmax"), (m, "k_minmax_partial", "nsplit=1"), (m, "k_minmax_partial", "nsplit>1"),
         (m + "_pt", "k_minmax_partial", "nsplit=1_pt"), (m + "_pt", "k_minmax_partial", "nsplit>1_pt")}
    V |= {(f, "k_small_rows_fused", "epl%d" % e) for e in (1, 2, 3, 4, 8)}
    V |= {(f, "k_rows_reg", "L%dx%d" % p) for p in REG_PAIRS}
    V |= {(f, "k_rows_staged", "group%d" % g) for g in (1, 2, 4, 8)}
    V |= {(m, "k_rows_staged_mm", "group%d" % g) for g in (1, 2, 4, 8)}
    V |= {(m, "k_rows_reg", "phase%d" % p) for p in range(4)}
    return V


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
FUSED_SPECIAL = ("nan", "+inf", "-inf", "+0", "-0", "mixed0", "positive", "negative", "denormal")
FINITE_SPECIAL = ("+0", "-0", "mixed0", "positive", "negative", "denormal")


def row_ranges(fmt, C, op, seed=0):
    """the range of every row: ranges(fmt) in turn (quantize: the maxval handed to the kernel; the degenerate ones -- 0, NaN,
    inf, denormal, huge -- so have rows of their own); one range for a per-tensor call"""
    R = ranges(fmt)
    if not pc_of(op):
        return [R[0]] * C
    return [R[(r + seed) % len(R)] for r in range(C)]


def fused_kinds(fmt, C, seed=0, per_channel=True, nan=False):
    """(kind, range) of every row of a fused / min-max case: the finite positive ranges of the format in turn, then the rows that
    are special as a whole.  A per-tensor min/max has one result for all rows, which a NaN or an infinity anywhere would own: its
    rows are the finite kinds only, and nan=True is the separate case whose row 1 % C carries a NaN."""
    plain = [v for v in ranges(fmt) if is_plain(v)]
    kinds = [("plain", v) for v in plain] + [(k, plain[0]) for k in (FUSED_SPECIAL if per_channel else FINITE_SPECIAL)]
    out = [kinds[(r + seed) % len(kinds)] for r in range(C)]
    if nan:
        out[1 % C] = ("nan", plain[0])
    return out


def _edge_positions(C, inner, n_edges):
    """flat positions and edge indices: edge_slots' layout over the rows, then BORDER values on each side of every chunk border
    (the later write wins where the two meet)"""
    pos, slot = edge_slots((C, 1, inner), n_edges)
    idx = edge_index(slot, n_edges)
    n = C * inner
    b = np.arange(CHUNK, n, CHUNK, dtype=np.int64)
    if b.size:
        off = np.arange(-BORDER, BORDER, dtype=np.int64)
        bpos = (b[:, None] + off[None, :]).reshape(-1)
        # the values walk the list along the borders, the side after a border half a list ahead of the side before it
        bidx = (np.arange(b.size, dtype=np.int64)[:, None] * BORDER + (off % BORDER)[None, :] + np.where(off >= 0, n_edges // 2, 0)[None, :]).reshape(-1) % n_edges
        keep = (bpos >= 0) & (bpos < n)
        pos, idx = np.concatenate([pos, bpos[keep]]), np.concatenate([idx, bidx[keep]])
    # the last write of a position wins: keep that one only
    _, last = np.unique(pos[::-1], return_index=True)
    sel = np.sort(pos.size - 1 - last)
    return pos[sel], idx[sel]


def case_input(shape, fmt, op, seed=0, nan=False):
    """dict(x [C, inner] float32, maxval [C] or [1] (quantize), ranges (per row), pos, idx, val, kinds) of one case.
    pos / idx / val: x.flat[pos] == val bit for bit, val = edge value idx of the row's own range (fused and min/max rows: only the
    finite values that do not exceed the row's range; the others keep their normal).

    quantize   normals scaled to range / 2.3 (range 1 where it is 0, inf or NaN), the edge values of the row's range laid over them.
    fused      the row's range is its own abs-max: +-range is planted (sign and place change with the row) and everything else stays
               at or below it, so that a default range gives an integer bias and real ties; rows of their own carry a NaN, +inf,
               -inf, all +0, all -0, mixed signed zeros, one-sided data, denormals only.
    min/max    the fused rows (seed picks another batch); the planted extreme sits in turn at the row's first element -- for rows
               that do not start a 16-byte group, a head element that shares its group with the row before --, at its last, and
               just before and just after a chunk border where the row has one."""
    mbits, n_bits, sign_bits = fmt
    C, inner = shape
    rng = np.random.RandomState(seed)
    bop = base_op(op)
    n_edges = len(edge_values(mbits, 1.0, sign_bits, n_bits))
    pos, idx = _edge_positions(C, inner, n_edges)
    row_of = pos // inner
    x = rng.randn(C, inner).astype(np.float32)
    xf = x.reshape(-1)
    if bop == "quantize":
        rr = row_ranges(fmt, C, op, seed)
        scale = np.array([r if is_plain(r) else 1.0 for r in rr], np.float64)
        with np.errstate(over="ignore", under="ignore"):
            x *= (scale / 2.3).astype(np.float32)[:, None]
        tables = {}
        val = np.empty(pos.size, np.float32)
        for s in np.unique(scale):
            tables[s] = edge_values(mbits, float(s), sign_bits, n_bits)
            sel = scale[row_of] == s
            val[sel] = tables[s][idx[sel]]
        xf[pos] = val
        mv = np.array(rr if pc_of(op) else rr[:1], np.float32)
        return dict(x=x, maxval=mv, ranges=rr, pos=pos, idx=idx, val=val, kinds=None)
    kinds = fused_kinds(fmt, C, seed, pc_of(op), nan)
    rr = [v for _, v in kinds]
    scale = np.array(rr, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        x *= (scale / 2.3).astype(np.float32)[:, None]
        lim = scale.astype(np.float32)[:, None]
    np.clip(x, -lim, lim, out=x)
    val = np.zeros(pos.size, np.float32)
    keep = np.zeros(pos.size, bool)
    for s in np.unique(scale):
        ev = edge_values(mbits, float(s), sign_bits, n_bits)
        sel = scale[row_of] == s
        v = ev[idx[sel]]
        val[sel] = v
        with np.errstate(invalid="ignore"):
            keep[sel] = np.isfinite(v) & (np.abs(v) <= np.float32(s))
    pos, idx, val = pos[keep], idx[keep], val[keep]
    xf[pos] = val
    # the planted extreme and the special rows
    planted = np.zeros(C, np.int64)
    for r, (kind, s) in enumerate(kinds):
        row = x[r]
        first = r * inner
        places = [0, inner - 1]
        nb = -(-first // CHUNK) * CHUNK                      # the first chunk border at or after the row's start
        if first < nb < first + inner:
            places += [nb - first - 1, nb - first]
        p = places[(r + seed) % len(places)]
        sgn = -1.0 if (sign_bits and (r + seed) % 2) else 1.0
        if kind == "+0":
            row[:] = 0.0
        elif kind == "-0":
            row[:] = -0.0
        elif kind == "mixed0":
            row[:] = np.where(rng.rand(inner) < 0.5, 0.0, -0.0).astype(np.float32)
        elif kind == "positive":
            np.abs(row, out=row)
        elif kind == "negative":
            np.negative(np.abs(row), out=row)
            sgn = -1.0
        elif kind == "denormal":
            row[:] = (rng.randint(-(1 << 20), 1 << 20, inner).astype(np.float64) * 2.0 ** -149).astype(np.float32)
        if kind in ("plain", "positive", "negative", "nan", "+inf", "-inf"):
            row[p] = np.float32(sgn * s)
        if kind == "nan":
            row[(p + inner // 2) % inner if inner > 1 else 0] = np.nan
        elif kind == "+inf":
            row[(p + inner // 2) % inner if inner > 1 else 0] = np.inf
        elif kind == "-inf":
            row[(p + inner // 2) % inner if inner > 1 else 0] = -np.inf
        planted[r] = p
    # what the special rows overwrote is no longer an edge value of the case
    ok = xf[pos].view(np.int32) == val.view(np.int32)
    return dict(x=x, maxval=None, ranges=rr, pos=pos[ok], idx=idx[ok], val=val[ok], kinds=kinds, planted=planted)


def tie_cloud(fmt, C, inner, seed):
    """rows filled with values within a few ulp of the rounding ties of their own range, for ranges whose bias is no integer (the
    grid step is then no power of two and its reciprocal is inexact): where a quotient formed with the reciprocal lands on the
    other side of the tie than the division does.  Every binade of epilogue_cases.ties, the first one included."""
    rng = np.random.RandomState(seed)
    R = [0.7361, 2.5, 0.0123, 1.37, 0.3333, 57.1, 1e-3, 9.9]
    mv = np.array([R[r % len(R)] for r in range(C)], np.float32)
    x = np.empty((C, inner), np.float32)
    for r in range(C):
        t = np.array([v for _, _, v, _ in ties(fmt[0], float(mv[r]), fmt[2], fmt[1])], np.float64)
        t = t[t <= float(mv[r])]
        first = np.array([v for p, _, v, _ in ties(fmt[0], float(mv[r]), fmt[2], fmt[1]) if p == 1], np.float64)
        t = np.concatenate([t, np.resize(first, t.size)])        # half of the picks from the first binade
        pick = t[rng.randint(0, t.size, inner)] * (1.0 + rng.randint(-6, 7, inner) * 2.0 ** -24)
        x[r] = (pick * rng.choice([-1.0, 1.0] if fmt[2] else [1.0], inner)).astype(np.float32)
    return x, mv
