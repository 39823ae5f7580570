"""Shared builders of the chunked kernels' tests (tests/test_chunk_routes_host.py, tests/test_chunk_routes_gpu.py): the shapes
with the route fields each must reach (ops.chunk_route), and the inputs.  A helper, not a test module; numpy only, needs no GPU.

The geometry under test (csrc/fp8q_intq.h): a block owns one aligned 4096-element chunk, builds the constants of the nc rows
overlapping it in nc_max = min(4096 / inner + 2, C) float4 of LDS (256 lanes, `i += 256`), and finds an element's row by
(phase + off) / inner -- magic division below a chunk, `l >= inner` from a chunk on.

  SHAPES     (C, inner, per_channel) -> the fields of ops.chunk_route the shape must find (aligned fp32 pointers)
  SIGN_C     the two row counts around kSignInline, as [C, 2] tensors; sign_inputs(C): the x_min vectors
  UNALIGNED  the shapes repeated with pointers off a 16-byte boundary
  int_case / ocp_case   x and the ranges: every row has its own range, neighbouring rows differ by at least two orders of
             magnitude, row 1 is degenerate (x_min == x_max == 0; OCP: maxval 0) and row 2 has a positive minimum; the lane's
             edge values lie over the first and last elements of every row (rotated by the row, cycled across rows shorter than
             the list) and on both sides of every 4096-element border
  int_consts / int_levels / int_values   the uniform quantizer's CPU chain in numpy float32, with the row of every element as
             an argument, so that a host test can recompute a case with a wrong row index
  rows_true / rows_* the row of every element: as the kernels must find it, and under each plausible fault
"""
import numpy as np

CHUNK = 4096
BLOCK = 256
SIGN_INLINE = 2048
BORDER = 8                   # planted elements on each side of a chunk border
EPS = 1e-8
f32 = np.float32


def _r(grid_x, rows, last, two_row=False, pc=True):
    return dict(grid_x=grid_x, rows_per_chunk=rows, lds_bytes=16 * rows, last_chunk=last, two_row=two_row, per_channel=pc,
                vec=True, nontemporal=False, sign_prepass=False)


SHAPES = {
    # one pass / two passes of the row setup
    (600, 16, True): _r(3, 258, 1408),             # 256 rows in every full chunk, rows aligned to chunks
    (600, 15, True): _r(3, 275, 808),              # 274 / 275 rows
    # many passes, rows straddling every border
    (2800, 3, True): _r(3, 1367, 208),
    (1700, 5, True): _r(3, 821, 308),
    # the tight LDS bound: chunk 11 has phase 22 and overlaps 1 + 178 + 1 rows
    (2140, 23, True): _r(13, 180, 68),
    # inner == 1
    (4096, 1, True): _r(1, 4096, 4096),
    (4097, 1, True): _r(2, 4097, 1),
    (8203, 1, True): _r(3, 4098, 11),              # 65,568 bytes of LDS; the last chunk: two groups and a 3-element tail
    (4101, 2, True): _r(3, 2050, 10),
    # around a chunk
    (5, 4095, True): _r(5, 3, 4091),               # magic division up to l = 8189
    (5, 4096, True): _r(5, 3, 4096, two_row=True),
    (5, 4097, True): _r(6, 2, 5, two_row=True),
    # per tensor
    (1, 12291, False): _r(4, 1, 3, pc=False),
    # the sign border (their sign_prepass is asserted with symmetric, range-setting queries)
    (2048, 2, True): _r(1, 2048, 4096),
    (2049, 2, True): _r(2, 2049, 2),
}
SIGN_C = (SIGN_INLINE, SIGN_INLINE + 1)
UNALIGNED = [(8203, 1, True), (2140, 23, True), (5, 4097, True)]
WIDE_BITS = [(4097, 1, True), (8203, 1, True), (2140, 23, True)]      # these also run at 2 and 16 bits
TIGHT = (2140, 23, 11)       # (C, inner, chunk): the chunk whose row count meets the bound


def route_of(ops, key, **kw):
    C, inner, pc = key
    return ops.chunk_route(C, inner, pc, **kw)


def completeness(key, r):
    """the values of the completeness list a route stands for"""
    rows = r["rows_per_chunk"]
    out = {"rows<=256" if rows <= BLOCK else "rows>256", "two_row" if r["two_row"] else "!two_row",
           "vec" if r["vec"] else "!vec", "sign_prepass" if r["sign_prepass"] else "!sign_prepass"}
    if rows > CHUNK:
        out.add("rows>4096")
    if r["per_channel"] and rows == CHUNK // key[1] + 2:
        out.add("rows==bound")
    last = r["last_chunk"]
    out.add("last_full" if last == CHUNK else ("last_groups" if last % 4 == 0 else "last_tail"))
    return out


COMPLETE = {"rows<=256", "rows>256", "rows==bound", "rows>4096", "two_row", "!two_row", "vec", "!vec", "sign_prepass",
            "!sign_prepass", "last_full", "last_groups", "last_tail"}


def chunk_rows(C, inner, chunk):
    """(first row, rows) a chunk of a [C, inner] tensor overlaps, counted element by element"""
    e0, e1 = chunk * CHUNK, min((chunk + 1) * CHUNK, C * inner)
    rows = np.unique(np.arange(e0, e1, dtype=np.int64) // inner)
    return int(rows[0]), int(rows.size)


# ---------------------------------------------------------------------------------------------------------------------------
# the row of every element
# ---------------------------------------------------------------------------------------------------------------------------
def rows_true(C, inner):
    return np.arange(C * inner, dtype=np.int64) // inner


def rows_border_one_low(C, inner):
    """the row index one too low for the first element after a chunk border"""
    rows = rows_true(C, inner)
    b = np.arange(CHUNK, C * inner, CHUNK)
    rows[b] = np.maximum(rows[b] - 1, 0)
    return rows


def rows_phase_zero(C, inner):
    """the phase of a chunk's first row taken as 0: row = c_lo + off / inner"""
    e = np.arange(C * inner, dtype=np.int64)
    e0 = e // CHUNK * CHUNK
    return np.minimum(e0 // inner + (e - e0) // inner, C - 1)


def rows_last_entry_missing(C, inner, nc_max):
    """the constants of LDS entry nc_max - 1 missing: its elements get the entry before it"""
    e = np.arange(C * inner, dtype=np.int64)
    local = e // inner - e // CHUNK * CHUNK // inner
    return np.where(local == nc_max - 1, e // inner - 1, e // inner)


# ---------------------------------------------------------------------------------------------------------------------------
# the uniform quantizer's CPU chain, numpy float32 (quantization/uniform.py: set_quant_range, to_integer_forward, forward)
# ---------------------------------------------------------------------------------------------------------------------------
def sign_of(xmin, first=None):
    """the symmetric quantizer's sign: min(x_min, 0).min() < 0, false with a NaN; first: folded from that many entries only"""
    v = np.minimum(np.asarray(xmin, f32).reshape(-1)[:first], f32(0))
    return bool(not np.isnan(v).any() and (v < 0).any())


def int_consts(xmin, xmax, n_bits, sym, sign=None, eps=EPS):
    """dict(scale, zp [C], lo, hi, delta, zf, sign) of set_quant_range(xmin, xmax); sign: override the symmetric sign"""
    xmin, xmax = np.asarray(xmin, f32).reshape(-1), np.asarray(xmax, f32).reshape(-1)
    with np.errstate(all="ignore"):
        mn = np.where(np.isnan(xmin), xmin, np.minimum(xmin, f32(0)))
        mx = np.where(np.isnan(xmax), xmax, np.maximum(xmax, f32(eps)))
        if sym:
            sign = sign_of(xmin) if sign is None else bool(sign)
            hi = f32(2.0 ** (n_bits - sign) - 1)
            lo = f32(-(2.0 ** (n_bits - 1))) if sign else f32(0)
            delta = (np.maximum(np.abs(mn), mx) / hi).astype(f32)
            delta = np.where(np.isnan(mn) | np.isnan(mx), f32(np.nan), delta)
            zf = np.zeros_like(delta)
            zp = np.zeros_like(delta)
        else:
            sign, lo, hi = False, f32(0), f32(2.0 ** n_bits - 1)
            delta = ((mx - mn) / hi).astype(f32)
            zf = (-mn / delta).astype(f32)
            zp = np.clip(np.rint(zf), lo, hi).astype(f32)
        scale = np.where(np.isnan(delta), delta, np.maximum(delta, f32(eps))).astype(f32)
    return dict(scale=scale, zp=zp, lo=lo, hi=hi, delta=delta, zf=zf, sign=sign)


def int_levels(x, k, rows):
    """clamp(rint(x / scale) + zp, lo, hi) with the constants of rows[e] for element e"""
    x = np.asarray(x, f32).reshape(-1)
    with np.errstate(all="ignore"):
        q = (np.rint((x / k["scale"][rows]).astype(f32)) + k["zp"][rows]).astype(f32)
        return np.clip(q, k["lo"], k["hi"]).astype(f32)


def int_values(x, k, rows):
    with np.errstate(all="ignore"):
        return (k["scale"][rows] * (int_levels(x, k, rows) - k["zp"][rows])).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
_DECADES = np.array([-3, 1, -1, 3, -2, 2, 0])      # neighbours (and the wrap) differ by two decades or more


def magnitudes(C):
    return (10.0 ** _DECADES[np.arange(C) % 7]).astype(f32)


def int_ranges(C, pc=True):
    """(x_min, x_max) [C] (per tensor: [1])"""
    if not pc:
        return np.array([-2.75], f32), np.array([3.5], f32)
    r = np.arange(C)
    m = magnitudes(C)
    xmin = (-m * (0.6 + 0.05 * (r % 5))).astype(f32)
    xmax = (m * (1.0 + 0.1 * (r % 3))).astype(f32)
    if C > 2:
        xmin[1] = xmax[1] = 0.0                   # degenerate: the scale is eps
        xmin[2] = 0.25 * m[2]                     # a positive minimum: the range still contains 0
    return xmin, xmax


def int_edges(k):
    """[C, n] the INT lane's edge values of every row: exact ties (k + 1/2) * scale with both float neighbours, both clamp ends
    and one step beyond, +-0, +-inf, denormals, +-1e30 and a NaN"""
    s, zp = k["scale"].astype(np.float64), k["zp"].astype(np.float64)
    lo, hi = float(k["lo"]), float(k["hi"])
    cols = []
    with np.errstate(all="ignore"):
        for j in (0.5, 1.5, -1.5):
            # ties on both sides of zero; for grids that start at 0 the negative one clamps, which is an edge of its own
            t = (j * s).astype(f32)
            cols += [t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf))]
        cols += [((hi - zp - 0.5) * s).astype(f32)]                                       # the last tie below the upper end
        cols += [((lo - zp) * s).astype(f32), ((lo - zp - 1) * s).astype(f32), ((hi - zp) * s).astype(f32),
                 ((hi - zp + 1) * s).astype(f32)]
    C = s.size
    for v in (0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1e30, -1e30, np.nan):
        cols.append(np.full(C, v, f32))
    return np.stack(cols, axis=1)


OCP_FMAX = {"e4m3fn": 448.0, "e5m2": 57344.0}
OCP_SUB = {"e4m3fn": 2.0 ** -9, "e5m2": 2.0 ** -16}


def ocp_ranges(C, pc=True):
    if not pc:
        return np.array([3.0], f32)
    mv = (magnitudes(C) * (0.75 + 0.05 * (np.arange(C) % 4))).astype(f32)
    if C > 2:
        mv[1] = 0.0                                # degenerate: the scale is eps / fmax
    return mv


def ocp_edges(maxval, fmt):
    """[C, n] the values tests/test_ocp_gpu.py plants, for every row's range"""
    mv = np.asarray(maxval, f32)
    s = np.maximum(mv, f32(EPS)).astype(np.float64) / OCP_FMAX[fmt]
    sub = OCP_SUB[fmt]
    up = np.nextafter(mv, f32(np.inf))
    C = mv.size
    cols = [np.full(C, v, f32) for v in (0.0, -0.0, np.inf, -np.inf, np.nan)]
    with np.errstate(all="ignore"):
        cols += [mv, -mv, up, -up, (2 * mv).astype(f32)]
        cols += [(c * sub * s).astype(f32) for c in (0.4999, -0.4999, 0.5, -0.5001, 1.5, -2.5)]
    cols += [np.full(C, v, f32) for v in (1e-45, -1e-45)]
    cols += [(0.3 * np.maximum(mv, f32(EPS))).astype(f32)]                  # OCP_SENS: a plain value inside the range
    return np.stack(cols, axis=1)


INT_SENS = 3      # the edges whose result differs under any neighbour's constants: the tie 1.5 * scale, a plain in-range value
OCP_SENS = 18


def plant(C, inner, n, sens):
    """(pos, idx): the flat positions that hold an edge value and which of the n edges each holds.  Rows at least n long: the
    first ceil(n / 2) and last floor(n / 2) elements, the list rotated by the row; shorter rows: every element, the list cycled
    across rows; and BORDER elements on both sides of every chunk border, the two elements at the border itself holding edge
    `sens` (as the tensor's last element does), whose result depends on the row's constants (a zero or an infinity there would hide a wrong row)."""
    N = C * inner
    e = np.arange(N, dtype=np.int64)
    row, j = e // inner, e % inner
    if inner >= n:
        h = (n + 1) // 2
        first, last = j < h, j >= inner - (n - h)
        mask = first | last
        idx = np.where(first, j, n - (inner - j)) + 3 * row
    else:
        mask = np.ones(N, bool)
        idx = e.copy()
    b = np.arange(CHUNK, N, CHUNK)
    near = np.zeros(N, bool)
    for d in range(-BORDER, BORDER):
        near[np.clip(b + d, 0, N - 1)] = True
    idx = np.where(near & ~mask, e, idx) % n
    idx[b] = idx[b - 1] = sens
    idx[N - 1] = sens                 # ... and the tensor's last element: the last LDS entry of a tensor with few rows
    mask |= near
    return e[mask], idx[mask]


def _fill(C, inner, mag, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((C, inner)) * mag.reshape(-1, 1)).astype(f32)


def int_case(key, n_bits=8, sym=False, seed=0):
    """dict(x [C, inner], xmin, xmax, pos, idx, rows): rows[e] the range entry of element e (0 per tensor)"""
    C, inner, pc = key
    xmin, xmax = int_ranges(C, pc)
    k = int_consts(xmin, xmax, n_bits, sym)
    rows = rows_true(C, inner) if pc else np.zeros(C * inner, np.int64)
    x = _fill(C, inner, 1.2 * np.abs(xmax) if pc else np.full(C, 4.0, f32), seed).reshape(-1)
    E = int_edges(k)
    pos, idx = plant(C, inner, E.shape[1], INT_SENS)
    x[pos] = E[rows[pos], idx]
    return dict(x=x.reshape(C, inner), xmin=xmin, xmax=xmax, pos=pos, idx=idx, rows=rows, n_edges=E.shape[1])


def ocp_case(key, fmt, seed=0):
    """dict(x [C, inner], maxval, pos, idx, rows)"""
    C, inner, pc = key
    mv = ocp_ranges(C, pc)
    rows = rows_true(C, inner) if pc else np.zeros(C * inner, np.int64)
    x = _fill(C, inner, 1.4 * mv if pc else np.full(C, 4.0, f32), seed).reshape(-1)
    E = ocp_edges(mv, fmt)
    pos, idx = plant(C, inner, E.shape[1], OCP_SENS)
    x[pos] = E[rows[pos], idx]
    return dict(x=x.reshape(C, inner), maxval=mv, pos=pos, idx=idx, rows=rows, n_edges=E.shape[1])


def sign_inputs(C):
    """name -> (x_min [C], the sign it folds to).  A fold that read only part of the vector gets one of them wrong."""
    m = (0.5 + 0.25 * (np.arange(C) % 7)).astype(f32)
    last_neg = m.copy()
    last_neg[C - 1] = -1.5
    mid_neg = m.copy()
    mid_neg[1500] = -1.5
    nan_last = -m
    nan_last[C - 1] = np.nan
    return {"last_negative": (last_neg, True), "negative_at_1500": (mid_neg, True), "nan_last": (nan_last, False),
            "non_negative": (m.copy(), False)}


def sign_case(C, name, seed=0):
    """a [C, 2] tensor under sign_inputs(C)[name]: dict(x, xmin, xmax, sign)"""
    xmin, sign = sign_inputs(C)[name]
    xmax = (2.0 + 0.5 * (np.arange(C) % 3)).astype(f32)
    x = _fill(C, 2, np.full(C, 2.5, f32), seed)
    return dict(x=x, xmin=xmin, xmax=xmax, sign=sign)
