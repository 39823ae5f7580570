"""Shared builders of the fused FP8 epilogue's tests (tests/test_epilogue_cases_host.py, tests/test_epilogue_cases_gpu.py): the
formats, the ranges of a format, the hand-picked hard inputs of one quantizer, the input tensors that carry them through a
batch norm / residual / activation unchanged, and the shapes with the kernel each must reach.  A helper, not a test module;
numpy only, needs no GPU.

  formats   (mbits, n_bits, sign_bits).  (7,8,1) and (8,8,0) have no exponent bit, (1,8,0) has seven, (2.5,8,1) and (3.5,8,1)
            round half to even to M = 2 and M = 4.
  ranges    the format's default maxval -- (2 - 2^-M) * 2^(2^E - 1 - B) with the integer B nearest 2^(E-1) for which the
            reference's float32 arithmetic returns the bias B exactly (default_maxval) -- then ordinary, tiny, denormal, huge,
            inf, 0 and NaN ones; with seven exponent
            bits also 1e-30, where the lowest scale 2^(1 - M - bias) underflows and the reference yields NaN.
  edges     edge_values: the recipe of tests/golden/make_golden.py:edge_inputs, restated (that script imports the reference).
  inputs    case_input: normals scaled to maxval / 2.3 with the edge values laid over the start and the end of every plane, so
            that they sit on both sides of every plane border and at every phase of a 16-byte group.  Behind a batch norm the
            constants are powers of two -- gamma = 2^k, k cycling over -2 .. 2 by channel, invstd = 1, mean = 0, beta = -0.0 --
            and the edge values are divided by gamma beforehand; a residual is -0.0 at the edge positions.  (-0.0, not +0.0:
            fma(x, alpha, +0.0) and t + 0.0 turn the edge value -0.0 into +0.0; adding -0.0 changes no float.)  A denormal edge
            value loses bits when divided by 4 and a huge one overflows when divided by 1/4, so k cycles over those of -2 .. 2
            that every finite edge value of the case survives (all five unless maxval is denormal or huge; a shape with
            C = 1 has the first of them, 2^-2 as a rule, as its only gamma): what
            tests/test_epilogue_cases_host.py proves for every case is that each edge value reaches the quantizer bit for bit.
            A tensor with fewer elements than edge values takes a window of the list that `start` moves; starts(shape, edges)
            lists the offsets at which the cases of a shape together hold every value at every phase of a 16-byte group.
  shapes    SHAPES: shape -> {has_bn: (kernel, direct, launches)} as ops.affine_act_route must report it.
"""
import numpy as np

FORMATS = [(3, 8, 1), (2, 8, 1), (4, 8, 1), (1, 8, 1), (7, 8, 1), (3, 8, 0), (8, 8, 0), (1, 8, 0), (2, 4, 1), (3, 6, 0),
           (2.5, 8, 1), (3.5, 8, 1)]

# (use_bn, use_res, act): the six flag sets of tests/test_epilogue.py
FLAGS = [(True, False, 1), (True, True, 1), (False, True, 1), (True, False, 2), (True, False, 0), (False, False, 0)]

_SMALL = ("small", False, 1)
SHAPES = {
    (2, 8, 5, 5): {True: _SMALL, False: _SMALL},                  # groups that cross one plane border
    (3, 40, 33, 31): {True: _SMALL, False: _SMALL},               # several blocks per image, ragged last one
    (1, 4, 256, 256): {True: _SMALL, False: _SMALL},              # HW beyond the 32-bit magic division's range
    (70000, 1, 2, 2): {True: ("small", False, 2), False: ("small", False, 2)},     # more images than gridDim.y: two launches
    (3, 12, 1, 1): {True: ("staged1", False, 1), False: _SMALL},  # HW = 1: four planes per group, constants in LDS
    (16, 5000): {True: ("staged1", False, 1), False: _SMALL},     # HW = 1: thousands of planes per piece
    (6, 4, 3, 1): {True: ("staged1", False, 1), False: _SMALL},   # HW = 3: groups crossing one or two planes
    (5, 2, 2, 1): {True: ("staged1", True, 1), False: _SMALL},    # C = 2, HW = 2: both planes in registers, p1 in mid-group
}


def nchw(shape):
    N, C = shape[0], shape[1]
    return N, C, int(np.prod(shape[2:], dtype=np.int64))


def fmt_me(fmt):
    """(M, E) of a format: mbits rounded half to even and clamped to [1, n_bits - sign_bits] (fp8_quantizer.py:105-107)"""
    mbits, n_bits, sign_bits = fmt
    M = int(min(max(np.rint(mbits), 1), n_bits - sign_bits))
    return M, n_bits - sign_bits - M


def bias32(fmt, maxval):
    """the quantizer's bias as the reference forms it (fp8_quantizer.py:105-110): ((2^E - log2(maxval)) + log2(2 - 2^-M)) - 1,
    every step rounded to float32"""
    M, E = fmt_me(fmt)
    f = np.float32
    b = f(2.0 ** E) - f(np.log2(np.float64(f(maxval))))
    b = b + f(np.log2(np.float64(f(2) - f(2.0 ** -M))))
    return f(b - f(1))


def default_maxval(fmt):
    """(2 - 2^-M) * 2^(2^E - 1 - B) for the integer B nearest 2^(E-1) (the usual IEEE-like bias; 0 for E = 0) at which
    the reference's float32 op chain returns the bias B EXACTLY: only then is the grid step a power of two and do rounding
    ties exist.  (At B = 2^(E-1) itself the chain is off by an ulp for M = 4, 7, 8 and for (3,6,0).)"""
    M, E = fmt_me(fmt)
    B0 = (1 << E) >> 1
    for d in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        mv = (2 - 2.0 ** (-M)) * 2.0 ** ((1 << E) - 1 - (B0 + d))
        if bias32(fmt, mv) == B0 + d:
            return float(mv)
    raise AssertionError("no integer bias near 2^(E-1) for %r" % (fmt,))


def ranges(fmt):
    out = [default_maxval(fmt), 2.5, 0.7361, 0.0123, 1e-40, 3e38, float("inf"), 0.0, float("nan")]
    if fmt_me(fmt)[1] == 7:
        out.append(1e-30)
    return out


def is_plain(maxval):
    """a finite positive range: the quantizer has a grid"""
    return bool(np.isfinite(maxval) and maxval > 0)


def _f32(v):
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(v)


def _neighbours(t):
    return [float(np.nextafter(t, np.float32(0))), float(np.nextafter(t, np.float32(np.inf)))]


TIE_K = lambda M: (0, 1, 2, 2 ** M - 1, 2 ** M, 2 ** M + 1, 2 ** (M + 1) - 2, 2 ** (M + 1) - 1)


def binades(E):
    pmax = 1 << E
    return [p for p in sorted({1, 2, 3, pmax // 2, pmax - 2, pmax - 1, pmax}) if p >= 1]


def ties(mbits, maxval, sign_bits, n_bits=8):
    """[(p, k, (k + 1/2) * s_p as float32, s_p)] of edge_values: s_p = 2^(p - M - bias) is the grid step of binade p"""
    M, E = fmt_me((mbits, n_bits, sign_bits))
    bias = 2.0 ** E - np.log2(float(np.float32(maxval))) + np.log2(2 - 2.0 ** (-M)) - 1
    out = []
    for p in binades(E):
        s = 2.0 ** (p - M - bias)
        out += [(p, k, _f32((k + 0.5) * s), s) for k in TIE_K(M)]
    return out


def edge_values(mbits, maxval, sign_bits, n_bits=8):
    """Hand-picked hard inputs of one quantizer (float32 array): +-0, tiny and denormal values, +-maxval and its two
    neighbours, +-1.5 maxval, +-inf, NaN; the rounding ties (k + 1/2) * s_p of the binades p in {1, 2, 3, pmax/2, pmax-2,
    pmax-1, pmax} with their neighbours and negatives; every such binade's lower edge with its neighbours and negative."""
    M, E = fmt_me((mbits, n_bits, sign_bits))
    mv = np.float32(maxval)
    bias = 2.0 ** E - np.log2(float(mv)) + np.log2(2 - 2.0 ** (-M)) - 1
    vals = [0.0, -0.0, 1e-30, -1e-30, 1e-42, float(mv), -float(mv), float(mv) * 1.5, -float(mv) * 1.5, float("inf"),
            float("-inf"), float("nan")] + _neighbours(mv)
    tie = ties(mbits, maxval, sign_bits, n_bits)
    for p in binades(E):
        for q, k, t, s in tie:
            if q == p:
                vals += [float(t)] + _neighbours(t) + [-float(t)]
        b = _f32(2.0 ** (p - bias))     # lower edge of binade p
        vals += [float(b)] + _neighbours(b) + [-float(b)]
    with np.errstate(over="ignore", under="ignore"):
        return np.array(vals, dtype=np.float32)


def gamma_exponents(edges):
    """those k of -2 .. 2 for which every finite edge value survives x = v / 2^k, t = x * 2^k bit for bit"""
    fin = edges[np.isfinite(edges)]
    keep = []
    for k in (-2, -1, 0, 1, 2):
        g = np.float32(2.0 ** k)
        with np.errstate(over="ignore", under="ignore"):
            back = (fin / g).astype(np.float32) * g
        if np.array_equal(back.view(np.int32), fin.view(np.int32)):
            keep.append(k)
    assert 0 in keep
    return keep


def cycle(n_edges):
    """length of the cycle the edge list is laid out in: the list and, to make it a multiple of 4, its first values again --
    so that a wrap of the cycle does not move a value's phase inside a 16-byte group by accident"""
    return -(-n_edges // 4) * 4


def edge_slots(shape, n_edges):
    """(flat positions, slot numbers) of the edge values in an [N, C, HW] tensor; slot s (plus the case's `start`) holds
    value edge_index(s, n_edges).  Plane q holds a + b = n = min(HW, cycle) of them, a at its start and b at its end.
    A plane that holds the whole cycle takes it from q * (HW + 1) on: a value then moves back by one phase of the 16-byte
    group from plane to plane whatever HW % 4 is, and meets all four phases within four planes.  Shorter planes continue
    where the plane before stopped, and every full pass over the cycle starts one value later, for the same reason."""
    N, C, HW = nchw(shape)
    L = cycle(n_edges)
    n = min(HW, L)
    a = (n + 1) // 2
    inside = np.concatenate([np.arange(a), np.arange(HW - (n - a), HW)]).astype(np.int64)
    q = np.arange(N * C, dtype=np.int64)[:, None]
    pos = (q * HW + inside[None, :]).reshape(-1)
    slot = (q * n + np.arange(n, dtype=np.int64)[None, :]).reshape(-1)
    slot = slot + (q * (HW + 1) + 0 * inside[None, :n]).reshape(-1) if n == L else slot + slot // L
    return pos, slot


def edge_index(slot, n_edges):
    return (slot % cycle(n_edges)) % n_edges


def starts(shape, n_edges):
    """the `start` offsets of the cases that one (shape, edge list) needs: one where the tensor holds the cycle four times
    over (every value then meets every phase of a group, see edge_slots); otherwise the windows that cover the cycle on a
    tensor smaller than it, each at the four phases"""
    numel = int(np.prod(shape, dtype=np.int64))
    L = cycle(n_edges)
    if numel >= 4 * L:
        return [0]
    return [r * numel + ph for r in range(-(-L // numel)) for ph in range(4)]


def case_input(shape, fmt, maxval, use_bn, use_res, seed=0, start=0, finite_only=False):
    """dict(x, bn, res, edges, placed, pos, idx) of one case (float32 numpy; bn = (mean, invstd, gamma, beta) or None): see the module
    docstring.  `edges` is the list the tensor draws from (a range that is 0, inf or NaN takes the list of maxval = 1;
    finite_only drops NaN and +-inf: the range twin's batches), `placed` those of it that the tensor holds: edges[idx] at the flat positions pos."""
    mbits, n_bits, sign_bits = fmt
    N, C, HW = nchw(shape)
    rng = np.random.RandomState(seed)
    scale = maxval if is_plain(maxval) else 1.0
    edges = edge_values(mbits, scale, sign_bits, n_bits)
    if finite_only:
        edges = edges[np.isfinite(edges)]
    with np.errstate(over="ignore", under="ignore"):
        x = (rng.randn(*shape) * (float(np.float32(scale)) / 2.3)).astype(np.float32)
        res = (rng.randn(*shape) * (float(np.float32(scale)) / 2.3)).astype(np.float32) if use_res else None
    pos, slot = edge_slots(shape, len(edges))
    idx = edge_index(start + slot, len(edges))
    xf = x.reshape(-1)
    xf[pos] = edges[idx]
    bn = None
    if use_bn:
        ks = gamma_exponents(edges)
        gamma = np.array([2.0 ** ks[c % len(ks)] for c in range(C)], np.float32)
        bn = (np.zeros(C, np.float32), np.ones(C, np.float32), gamma, np.full(C, -0.0, np.float32))
        ch = (pos // HW) % C
        with np.errstate(over="ignore", under="ignore"):
            xf[pos] = (edges[idx] / gamma[ch]).astype(np.float32)
    if use_res:
        res.reshape(-1)[pos] = -0.0
    placed = edges[np.unique(idx)]
    return dict(x=x, bn=bn, res=res, edges=edges, placed=placed, pos=pos, idx=idx)


def expected_t(case, act):
    """the pre-quantizer tensor act(bn(x) + residual): always the oracle's, never reasoned by hand"""
    import oracle
    return oracle.c_affine_act(case["x"], case["bn"], case["res"], act)


def same_bits(got, ref):
    """identical NaN masks, identical int32 bits elsewhere (the sign of zero included)"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    if got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), ref[~nan].view(np.int32)))
