"""K4 (the FP-MSE grid search) picks one of three kernels from the SHAPE of the call.  Every case here reaches its kernel by
shape, at the library's defaults (no environment variable is set), ASSERTS through ops.mse_route which kernel and which of
the launcher's size-dependent arms that is, and only then compares with the CPU oracle (oracle.c_mse_grid: plain C through
double libm, one quantizer pass per pair).  A threshold that moves fails the route assertion instead of quietly sending the
data built for one kernel through another.

Tolerance: K4's contract (include/fp8q.h), rtol 1e-5 on every entry, NaN / inf patterns exact.  Where data that sit on a
candidate's grid make an entry cancel, the absolute floor tests/test_mse_hist.py uses: 1e-24 x the table's largest entry.
"""
import numpy as np
import pytest
import torch

import oracle

GRID, ROW, HIST = 0, 1, 2            # fp8q_mse_route_info.kernel
NONE, FINAL_TILE, FINAL = 0, 1, 2    # .finish
ROW_TILE = 4096                      # kMseRowTile (csrc/fp8q_mse.hip): elements per wave and tile of k_mse_row
PART_TILE = 8192                     # kPartTile (csrc/fp8q_mse_hist.hip): keys per partition tile
SORT_LDS = 4096                      # kSortLds: borders of one coarse bucket that are sorted in LDS
MB6 = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
MB7 = MB6 + [7.0]


@pytest.fixture(scope="module")
def ops():
    import fp8q
    fp8q.lib()  # raises if libfp8q_hip.so is missing: no fallback
    return fp8q.ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def assert_table(got, ref, what, floor=False, scale=1.0):
    """got (the kernel's table) against scale * ref (the oracle's): NaN and inf patterns exactly, finite entries to 1e-5"""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32) * np.float32(scale)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), f"{what}: inf pattern"
    ok = np.isfinite(ref)
    atol = 1e-24 * float(got[ok].max()) if floor and ok.any() else 0.0
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-5, atol=atol, err_msg=what)


def assert_same_decision(got, ref, what):
    """the decision the estimator takes from the table: the oracle's argmin, or within 1e-6 of its minimum"""
    for c in range(ref.shape[2]):
        g, r = got[:, :, c], ref[:, :, c]
        gi, ri = np.unravel_index(np.argmin(g), g.shape), np.unravel_index(np.argmin(r), r.shape)
        assert gi == ri or r[gi] <= r[ri] * (1 + 1e-6), (what, c, gi, ri)


def run_grid(ops, x, per_channel, grid, mb, sign, calls=1):
    """the table after `calls` accumulating calls on a zeroed table"""
    C = grid.shape[1]
    mses = torch.zeros(len(mb), grid.shape[0], C, device="cuda")
    gd = grid if isinstance(grid, torch.Tensor) else dev(grid)
    for _ in range(calls):
        ops.mse_grid(x, per_channel, gd, mb, 8, sign, mses)
    return mses.cpu().numpy()


# ---- host: the route table -------------------------------------------------------------------------------------------------
def test_route_table_host():
    """The documented rule (include/fp8q.h, K4), no GPU needed: rows < 2048 elements take k_mse_grid, longer ones k_mse_row,
    per-tensor rows of >= 16384 elements with <= 4096 pairs and 8-bit formats the histogram."""
    import fp8q
    from fp8q._lib import MseRouteInfo
    import ctypes
    route = fp8q.ops.mse_route
    table = [((1, 2047), 111, MB6, GRID), ((1, 2048), 111, MB6, ROW), ((1, 16383), 111, MB6, ROW), ((1, 16384), 111, MB6, HIST),
             ((2, 16384), 111, MB6, ROW), ((1, 16384), 4097, [3.0], ROW), ((1, 16384), 4096, [3.0], HIST)]
    for (C, inner), n_cand, mb, kernel in table:
        for sign in (1, 0):
            assert route(C, inner, n_cand, mb, 8, sign)["kernel"] == kernel, (C, inner, n_cand, len(mb), sign)
    # nine widths: kHistMaxM is 8 -- and so is kMseMaxM, K4's own limit, which fp8q_mse_grid_f32 checks first: such a call never
    # reaches the histogram (or any kernel), it is an argument error
    L = fp8q.lib()
    info = MseRouteInfo()
    info.kernel = -1
    mb9 = (ctypes.c_float * 9)(*[float(m) for m in range(1, 10)])
    assert L.fp8q_mse_route(1, 16384, 111, mb9, 9, 8, 1, ctypes.byref(info)) == -1 and info.kernel != HIST
    assert route(1, 16384, 111, MB7 + [7.0], 8, 0)["kernel"] == HIST       # (eight widths are taken)
    for inner in (16384, 1 << 20):                                         # a 10-bit format: the cell tables are sized for 8 bits
        assert route(1, inner, 111, [3.0, 4.0], 10, 1)["kernel"] == ROW
    # the finishing launch: k_mse_row leaves one partial sum per 4096-element tile; up to 32 per row k_mse_final_tile adds them
    r = route(2, 32 * ROW_TILE, 111, [2.0, 3.0], 8, 1)
    assert (r["kernel"], r["nsplit"], r["finish"]) == (ROW, 32, FINAL_TILE)
    r = route(2, 32 * ROW_TILE + 1, 111, [2.0, 3.0], 8, 1)
    assert (r["kernel"], r["nsplit"], r["finish"]) == (ROW, 33, FINAL)
    r = route(960, 9, 111, [3.0], 8, 1)                                    # one split: k_mse_grid writes the table itself
    assert (r["kernel"], r["nsplit"], r["finish"]) == (GRID, 1, NONE)
    r = route(160, 960, 111, [3.0], 8, 1)                                  # (tests/test_cabi_and_host.py: 15 tiles of 64 elements)
    assert (r["kernel"], r["nsplit"], r["finish"]) == (GRID, 15, FINAL_TILE)
    r = route(1, 16384, 111, MB6, 8, 1)
    assert (r["finish"], r["nsplit"]) == (NONE, 0)
    assert (r["tiles_per_wg"], r["part_wgs"], r["slice_min"], r["moments_threads"], r["top_scan"]) == (1, 2, 2048, 512, 0)
    assert r["n_superblocks"] == -(-(666 * 195 + 2048 + 1) // 1024)        # 195 cells per candidate (M = 1 and M = 6), 2048 buckets
    # the partial sums the workspace holds follow nsplit
    for C, inner in ((2, 32 * ROW_TILE), (2, 33 * ROW_TILE + 5), (160, 960), (3, 5000)):
        r = route(C, inner, 111, [2.0, 3.0], 8, 1)
        assert L.fp8q_mse_workspace_bytes(C, inner, 111, 2) == C * 2 * 111 * r["nsplit"] * 8 + 16, (C, inner)
    # argument errors, as fp8q_mse_grid_f32 reports them
    one = (ctypes.c_float * 1)(3.0)
    rc = lambda *a: L.fp8q_mse_route(*a, ctypes.byref(info))
    assert rc(0, 5, 111, one, 1, 8, 1) == -1 and rc(1, 0, 111, one, 1, 8, 1) == -1 and rc(1, 5, 0, one, 1, 8, 1) == -1
    assert rc(1, 5, 111, one, 0, 8, 1) == -1 and rc(1, 5, (1 << 20) + 1, one, 1, 8, 1) == -1
    assert rc(1, 5, 111, None, 1, 8, 1) == -1 and L.fp8q_mse_route(1, 5, 111, one, 1, 8, 1, None) == -1
    assert rc(1, 5, 111, one, 1, 8, 2) == -1 and rc(1, 5, 111, one, 1, 1, 1) == -1
    assert rc(1, 5, 111, (ctypes.c_float * 1)(float("nan")), 1, 8, 1) == -1
    assert rc(65536, 5, 111, one, 1, 8, 1) == -5                           # FP8Q_ETOOMANY: gridDim.z
    assert rc(1, 5, 111, one, 1, 16, 1) == -2                              # FP8Q_EUNSUPPORTED: 12 exponent bits
    with pytest.raises(fp8q.Fp8qError):
        route(65536, 5, 111, [3.0], 8, 1)


# ---- k_mse_row, reached by shape ------------------------------------------------------------------------------------------
KINDS = ("relu", "negzero", "tiny", "beyond", "covered", "ties", "const", "sparse", "plain")


def _piece(kind, rng, L):
    """L elements of one kind of the tile recipe (test_hip_parity.py::test_mse_row_kernel_tile_dependent_paths)"""
    t = rng.randn(L).astype(np.float32)
    if kind == "relu":
        t *= (rng.rand(L) < 0.5)                                  # ReLU-like: half exact zeros
    elif kind == "negzero":
        t[::7] = -0.0
    elif kind == "tiny":
        t[:5] = np.float32([1e-6, -3e-7, 1e-20, 1e-38, 1e-45])    # tiny and denormal nonzeros: float path for every candidate
    elif kind == "beyond":
        t *= 8.0                                                  # far beyond most candidates: everything clamps
    elif kind == "covered":
        t *= 0.01                                                 # every candidate covers the piece: clamp-free
    elif kind == "ties":
        t = (np.round(t * 8) / 8 + 1 / 16).astype(np.float32)     # exact ties of coarse grids
    elif kind == "const":
        t[:] = 1.25
    elif kind == "sparse":                                        # nearly empty
        t[100] = 1e-3
        t[101:] = 0.0
    elif kind == "pinf":
        t[3] = np.inf
    elif kind == "ninf":
        t[5] = -np.inf
    else:
        assert kind == "plain"
    return t


def _row(kinds, rng, L, tail=5):
    return np.concatenate([_piece(k, rng, L) for k in kinds] + [rng.randn(tail).astype(np.float32)])


# per-tensor rows of 3 x 4096 + 5 elements: three whole tiles of one kind each, or six 2048-element halves (a tile's
# statistics -- its smallest nonzero, its largest element -- then come from two kinds)
PT_WHOLE = [("relu", "negzero", "tiny"), ("beyond", "covered", "ties"), ("const", "sparse", "plain")]
PT_HALF = [("relu", "beyond", "negzero", "covered", "tiny", "ties"), ("const", "plain", "sparse", "beyond", "covered", "relu")]
PT_WHOLE_INF = [("pinf", "ninf", "plain"), ("pinf", "beyond", "sparse")]
PT_HALF_INF = [("pinf", "plain", "relu", "ninf", "tiny", "beyond")]


@pytest.mark.gpu
@pytest.mark.parametrize("sign,special", [(1, False), (0, False), (1, True)])
@pytest.mark.parametrize("half", [False, True], ids=["tiles", "halves"])
def test_row_kernel_per_tensor_tile_paths(ops, half, sign, special):
    """k_mse_row on a per-tensor row below the histogram's threshold.  Per (tile, candidate) the kernel picks between integer
    rounding on the bits of t, the magic-number rounding and their clamp-free twins, with one or two scale mantissas, patches
    near-ties and has an exact path: the recipe's kinds of tile laid on the kernel's real tile of 4096 elements (and on halves
    of it), six widths x 111 candidates, signed, unsigned (one-sided data) and with +-inf."""
    L = ROW_TILE // 2 if half else ROW_TILE
    n = 3 * ROW_TILE + 5
    r = ops.mse_route(1, n, 111, MB6, 8, sign)
    assert r["kernel"] == ROW and r["nsplit"] == 4 and r["finish"] == FINAL_TILE, r
    rng = np.random.RandomState(23 + 2 * sign + half)
    grid = np.linspace(0.1 * 5.5, 1.2 * 5.5, 111).astype(np.float32)[:, None]
    for kinds in ((PT_HALF_INF if half else PT_WHOLE_INF) if special else (PT_HALF if half else PT_WHOLE)):
        x = _row(kinds, rng, L)
        assert x.size == n
        if sign == 0:
            x = np.abs(x)
        got = run_grid(ops, dev(x), False, grid, MB6, sign)
        ref = oracle.c_mse_grid(x, False, grid, MB6, 8, sign)
        assert_table(got, ref, f"{kinds} sign {sign}")
        assert_same_decision(got, ref, kinds)


@pytest.mark.gpu
@pytest.mark.parametrize("sign,special", [(1, False), (0, False), (1, True)])
@pytest.mark.parametrize("half", [False, True], ids=["tiles", "halves"])
def test_row_kernel_per_channel_tile_paths(ops, half, sign, special):
    """The same recipe on per-channel rows (k_mse_row serves every one of >= 2048 elements): C = 3, rows of 12 x 4096 + 5
    elements, every row with its own order of the kinds, its own scale and its own grid column."""
    C, inner = 3, 12 * ROW_TILE + 5
    r = ops.mse_route(C, inner, 111, MB6, 8, sign)
    assert r["kernel"] == ROW and r["nsplit"] == 13 and r["finish"] == FINAL_TILE, r
    rng = np.random.RandomState(41 + 2 * sign + half)
    scales = np.float32([1.0, 0.37, 16.0])                    # (powers of two keep the exact ties, 0.37 moves every border)
    L = ROW_TILE // 2 if half else ROW_TILE
    rows = []
    for c in range(C):
        kinds = list(KINDS) + ["plain"] * (12 - len(KINDS))
        if special:
            kinds[-1], kinds[-2] = "pinf", "ninf"
        if half:
            kinds = kinds + kinds[::-1]                       # every kind in a first and in a second half, next to another kind
            kinds = kinds[c:] + kinds[:c]
        else:
            kinds = list(np.roll(kinds, 4 * c))
        rows.append(_row(kinds, rng, L) * scales[c])
    x = np.stack(rows).astype(np.float32)
    assert x.shape == (C, inner)
    if sign == 0:
        x = np.abs(x)
    grid = (np.linspace(0.1 * 5.5, 1.2 * 5.5, 111).astype(np.float32)[:, None] * scales[None, :]).astype(np.float32)
    got = run_grid(ops, dev(x), True, grid, MB6, sign)
    ref = oracle.c_mse_grid(x, True, grid, MB6, 8, sign)
    assert_table(got, ref, f"sign {sign} special {special}")
    assert_same_decision(got, ref, (sign, special))


@pytest.mark.gpu
def test_row_kernel_nan(ops):
    """a NaN element makes every entry of its row NaN -- of its row only"""
    rng = np.random.RandomState(29)
    grid = np.linspace(0.1 * 5.5, 1.2 * 5.5, 111).astype(np.float32)[:, None]
    n = 3 * ROW_TILE + 5
    assert ops.mse_route(1, n, 111, [2.0, 3.0], 8, 1)["kernel"] == ROW
    x = rng.randn(n).astype(np.float32)
    x[2 * ROW_TILE + 77] = np.nan
    got = run_grid(ops, dev(x), False, grid, [2.0, 3.0], 1)
    assert np.isnan(got).all()
    assert_table(got, oracle.c_mse_grid(x, False, grid, [2.0, 3.0], 8, 1), "per tensor")
    C, inner = 3, 12 * ROW_TILE + 5
    assert ops.mse_route(C, inner, 111, [2.0, 3.0], 8, 1)["kernel"] == ROW
    x = rng.randn(C, inner).astype(np.float32)
    x[1, inner - 2] = np.nan                                  # in the ragged last tile of the middle row
    grid3 = grid * np.ones((1, C), np.float32)
    got = run_grid(ops, dev(x), True, grid3, [2.0, 3.0], 1)
    assert np.isnan(got[:, :, 1]).all() and np.isfinite(got[:, :, [0, 2]]).all()
    assert_table(got, oracle.c_mse_grid(x, True, grid3, [2.0, 3.0], 8, 1), "per channel")


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, 0])
def test_row_kernel_per_tensor_candidate_paths(ops, sign):
    """The candidate list of test_hip_parity.py::test_mse_row_kernel_all_paths -- 61 ranges over six decades, 1e-30, 1e-12,
    3e37, 0 and powers of two, seven widths -- on a per-tensor row that k_mse_row serves: the two-mantissa ranges and the
    exact path (tiny / huge / degenerate ranges) on C = 1."""
    rng = np.random.RandomState(11 + sign)
    n = 3 * ROW_TILE + 5
    r = ops.mse_route(1, n, 68, MB7, 8, sign)
    assert r["kernel"] == ROW and r["finish"] == FINAL_TILE, r
    x = (rng.randn(n) * 1.7).astype(np.float32)
    if sign == 0:
        x = np.abs(x)
    base = np.exp(np.linspace(np.log(2e-3), np.log(3e3), 61)).astype(np.float32)
    grid = np.concatenate([base, np.float32([1e-30, 1e-12, 3e37, 0.0, 1.0, 2.0, 4.0])])[:, None]
    grid = (grid * rng.uniform(0.9, 1.1, grid.shape)).astype(np.float32)
    assert grid.shape[0] == 68
    got = run_grid(ops, dev(x), False, grid, MB7, sign)
    ref = oracle.c_mse_grid(x, False, grid, MB7, 8, sign)
    assert np.isnan(ref[:, 64, 0]).all()                      # the zero candidate
    assert_table(got, ref, f"sign {sign}")


@pytest.mark.gpu
@pytest.mark.parametrize("inner,nsplit,finish", [(32 * ROW_TILE, 32, FINAL_TILE), (33 * ROW_TILE + 5, 34, FINAL)])
def test_row_kernel_finish_launches(ops, inner, nsplit, finish):
    """32 partial sums per row are the last count k_mse_final_tile adds up, 34 go to k_mse_final (a wave per table entry);
    two calls accumulate into one table."""
    C, mb = 2, [2.0, 3.0]
    r = ops.mse_route(C, inner, 111, mb, 8, 1)
    assert (r["kernel"], r["nsplit"], r["finish"]) == (ROW, nsplit, finish), r
    rng = np.random.RandomState(inner % 1000)
    x = (rng.randn(C, inner) * np.float32([[0.6], [2.2]])).astype(np.float32)
    grid = (np.linspace(0.1 * 4.5, 1.2 * 4.5, 111)[:, None] * np.float32([[0.6, 2.2]])).astype(np.float32)
    got = run_grid(ops, dev(x), True, grid, mb, 1, calls=2)
    ref = oracle.c_mse_grid(x, True, grid, mb, 8, 1)
    assert_table(got, ref, f"inner {inner}", scale=2.0)


# ---- the interval histogram, reached by shape ------------------------------------------------------------------------------
def _views(x):
    """x on the device three times: as allocated (16-byte aligned), and as the views buf[1:] and buf[3:] of a longer buffer
    (4-byte aligned only: whole partition tiles load 16-byte vectors)"""
    out = []
    for off in (0, 1, 3):
        buf = torch.zeros(x.size + off, device="cuda")
        v = buf[off:]
        v.copy_(torch.from_numpy(x))
        assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
        out.append(v)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sign,mb", [(1, MB6), (0, MB7)], ids=["signed6", "unsigned7"])
@pytest.mark.parametrize("n", [2 * PART_TILE, 2 * PART_TILE + 1, 3 * PART_TILE - 1])
def test_hist_smallest_sizes_and_alignments(ops, n, sign, mb):
    """The route's first sizes -- two whole partition tiles, one more element (a third tile of one key), a third tile one key
    short -- at the three alignments, every candidate against the oracle."""
    r = ops.mse_route(1, n, 111, mb, 8, sign)
    assert r["kernel"] == HIST and r["tiles_per_wg"] == 1 and r["part_wgs"] == -(-n // PART_TILE), r
    assert (r["slice_min"], r["moments_threads"], r["top_scan"]) == (2048, 512, 0), r
    rng = np.random.RandomState(n % 977 + sign)
    x = (rng.randn(n) * 1.3).astype(np.float32)
    if sign == 0:
        x = np.maximum(x, 0) - np.float32(0.01) * (rng.rand(n) < 0.01)      # ReLU output and a few negative elements (clipped to 0)
    x = x.astype(np.float32)
    grid = ops.mse_linspace(dev(np.abs(x).max().reshape(1)), 111)
    ref = oracle.c_mse_grid(x, False, grid.cpu().numpy(), mb, 8, sign)
    for v in _views(x):
        got = run_grid(ops, v, False, grid, mb, sign)
        assert_table(got, ref, f"n {n} offset {v.data_ptr() % 16}")
        assert_same_decision(got, ref, n)


def _degenerate(name, n, grid):
    x = np.zeros(n, np.float32)
    if name == "negzero":
        x[:] = -0.0
    elif name == "one":
        x[n // 3] = -1.7
    elif name == "denormal":
        x = (np.random.RandomState(3).randint(-(1 << 22), 1 << 22, n).astype(np.int32) & ~np.int32(0x7f800000)).view(np.float32).copy()
        x[x == 0] = np.float32(1e-45)
    elif name == "negative":
        x = -np.abs(np.random.RandomState(4).randn(n)).astype(np.float32) - np.float32(1e-3)
    elif name == "top":
        x[:] = grid[-1, 0]
    else:
        assert name == "zero"
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("name,sign", [("zero", 1), ("negzero", 1), ("negzero", 0), ("one", 1), ("one", 0), ("denormal", 1),
                                       ("negative", 0), ("top", 1), ("top", 0)])
def test_hist_degenerate_key_sets(ops, name, sign):
    """Key sets that leave the partition nearly or wholly empty at the smallest size: zeros of either sign (every key dropped),
    one nonzero element, denormals only (all keys in the first coarse buckets), all-negative data on an unsigned format (every
    key dropped, only the sum of the negative squares remains), every element on the largest candidate (one interval holds
    all keys; most entries are pure clamp errors, the last one cancels to 0).  The oracle decides, NaN pattern included."""
    n = 2 * PART_TILE
    mb = MB6 if sign else MB7
    assert ops.mse_route(1, n, 111, mb, 8, sign)["kernel"] == HIST
    grid = np.linspace(0.1 * 3.0, 1.2 * 3.0, 111).astype(np.float32)[:, None]
    x = _degenerate(name, n, grid)
    if name == "denormal":
        assert (np.abs(x) < np.float32(1.1754944e-38)).all() and (x != 0).all()
    if name == "negative":
        assert (x < 0).all()
    got = run_grid(ops, dev(x), False, grid, mb, sign)
    ref = oracle.c_mse_grid(x, False, grid, mb, 8, sign)
    assert_table(got, ref, name, floor=True)
    if name in ("zero", "negzero"):
        assert (got == 0).all()
    if name == "denormal":                                    # ... and with candidates of the data's own size (denormal ranges)
        grid = ops.mse_linspace(dev(np.abs(x).max().reshape(1)), 111)
        got = run_grid(ops, dev(x), False, grid, mb, sign)
        assert_table(got, oracle.c_mse_grid(x, False, grid.cpu().numpy(), mb, 8, sign), "denormal candidates", floor=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2 * PART_TILE + 77, (1 << 18) + 4099])
def test_hist_is_deterministic(ops, n):
    """integer moments, fixed-tree sums: the same call twice gives the same bits (include/fp8q.h promises it)"""
    assert ops.mse_route(1, n, 111, MB6, 8, 1)["kernel"] == HIST
    g = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(n, device="cuda", generator=g) * 0.8
    grid = ops.mse_linspace(x.abs().max().reshape(1), 111)
    a = run_grid(ops, x, False, grid, MB6, 1)
    b = run_grid(ops, x, False, grid, MB6, 1)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.int32), b.view(np.int32))


SUBSET = [0, 1, 40, 80, 109, 110]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True], ids=["gauss", "relu"])
def test_hist_two_tiles_per_workgroup_and_moments_256(ops, relu):
    """One tile more than the 768 partition workgroups have: every workgroup walks two tiles (the last one a ragged second
    tile), slices of 4096 keys, and above 3 M elements with <= 256 pairs k_moments runs with 256 threads.  ReLU data: the
    dropped zeros across a workgroup's tiles."""
    n = 768 * PART_TILE + PART_TILE + 77
    mb = [2.0, 3.0]
    r = ops.mse_route(1, n, 111, mb, 8, 1)
    assert r["kernel"] == HIST and (r["tiles_per_wg"], r["slice_min"], r["moments_threads"], r["top_scan"]) == (2, 4096, 256, 0), r
    assert r["part_wgs"] == 385
    g = torch.Generator(device="cuda").manual_seed(7 + relu)
    x = torch.randn(n, device="cuda", generator=g) * 1.3
    if relu:
        x = torch.relu(x)
    grid = ops.mse_linspace(x.abs().max().reshape(1), 111)
    got = run_grid(ops, x, False, grid, mb, 1)
    ref = oracle.c_mse_grid(x.cpu().numpy(), False, grid.cpu().numpy()[SUBSET], mb, 8, 1)
    assert_table(got[:, SUBSET, :], ref, "relu" if relu else "gauss")
    assert np.isfinite(got).all() and (got > 0).all()


@pytest.mark.gpu
def test_hist_largest_slice(ops):
    """beyond 2^24 elements the key slices stop growing (16384) and a partition workgroup walks three tiles"""
    n = (1 << 24) + 4099
    mb = [2.0, 3.0]
    r = ops.mse_route(1, n, 111, mb, 8, 1)
    assert r["kernel"] == HIST and (r["tiles_per_wg"], r["slice_min"], r["moments_threads"]) == (3, 16384, 256), r
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(n, device="cuda", generator=g) * 0.9
    grid = ops.mse_linspace(x.abs().max().reshape(1), 111)
    got = run_grid(ops, x, False, grid, mb, 1)
    idx = [40, 100]
    ref = oracle.c_mse_grid(x.cpu().numpy(), False, grid.cpu().numpy()[idx], mb, 8, 1)
    assert_table(got[:, idx, :], ref, "4 pairs")
    assert np.isfinite(got).all() and (got > 0).all()


def _borders_in_bucket(grid, M, sign, lo=2.0, hi=2.25, points=4096):
    """A LOWER bound of the cell borders that the candidates grid[:, 0] of width M put into the coarse bucket [lo, hi) (an
    eighth of a binade: the keys that share their top 11 bits): the oracle's quantizer is swept over `points` evenly spaced
    floats of the bucket, one row per candidate, and the places where its output changes are counted.  (A change is a
    border; a sweep that steps over a whole cell misses borders, it never invents one.)"""
    b0, b1 = np.float32(lo).view(np.int32), np.float32(hi).view(np.int32)
    assert (b0 >> 20) + 1 == (b1 >> 20)
    keys = np.arange(b0, b1, (b1 - b0) // points, dtype=np.int32).view(np.float32)
    sweep = np.ascontiguousarray(np.broadcast_to(keys, (grid.shape[0], keys.size)))
    y = oracle.c_quantize(sweep, grid[:, 0], M, 8, sign)
    return int((np.diff(y, axis=1) != 0).sum())


def _line_search_data(n):
    x = np.abs(np.random.RandomState(17).randn(n)).astype(np.float32)
    x *= np.float32(4.0) / x.max()                            # |N(0, 1)| with its maximum at 4
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("n_cand,top_scan", [(1000, 0), (2048, 1)])
def test_hist_global_sort_1000_candidates(ops, n_cand, top_scan):
    """More than kSortLds = 4096 borders in one coarse bucket: a line search's 1000 candidates (and 2048) of the unsigned
    M = 7 format put a few per candidate into [2, 2.25), and that bucket's borders are sorted by the bitonic network on global
    memory instead of in LDS.  Counted on the CPU first (twice kSortLds asked for: the count is a lower bound of what the
    kernel's exact borders come to, but it need not be close).  With 2048 candidates the prefix scan also has more than 512
    superblocks and k_iv_scan_top runs."""
    n = 2 * PART_TILE + 77
    r = ops.mse_route(1, n, n_cand, [7.0], 8, 0)
    assert r["kernel"] == HIST and r["top_scan"] == top_scan and (r["n_superblocks"] > 512) == bool(top_scan), r
    x = _line_search_data(n)
    grid = ops.mse_linspace(dev(x.max().reshape(1)), n_cand)
    gh = grid.cpu().numpy()
    assert _borders_in_bucket(gh, 7.0, 0) >= 2 * SORT_LDS
    assert ((x >= 2.0) & (x < 2.25)).sum() > 0                # ... and the bucket has keys to place among them
    got = run_grid(ops, dev(x), False, grid, [7.0], 0)
    ref = oracle.c_mse_grid(x, False, gh, [7.0], 8, 0)
    assert_table(got, ref, f"{n_cand} candidates")
    assert_same_decision(got, ref, n_cand)


@pytest.mark.gpu
def test_hist_line_search_signed(ops):
    """the line search as the reference runs it: 1000 candidates of the signed E1M6 format on the same data.  Whether its
    fullest bucket goes beyond the LDS sort is counted, not assumed; the comparison runs either way."""
    n = 2 * PART_TILE + 77
    r = ops.mse_route(1, n, 1000, [6.0], 8, 1)
    assert r["kernel"] == HIST and r["top_scan"] == 0, r
    x = _line_search_data(n) * np.where(np.random.RandomState(18).rand(n) < 0.5, -1, 1).astype(np.float32)
    grid = ops.mse_linspace(dev(np.abs(x).max().reshape(1)), 1000)
    gh = grid.cpu().numpy()
    borders = _borders_in_bucket(gh, 6.0, 1)
    print(f"\nsigned M = 6, 1000 candidates: >= {borders} borders in [2, 2.25) -> {'global' if borders >= 2 * SORT_LDS else 'LDS (or unproven)'} sort")
    got = run_grid(ops, dev(x), False, grid, [6.0], 1)
    ref = oracle.c_mse_grid(x, False, gh, [6.0], 8, 1)
    assert_table(got, ref, "signed line search")
    assert_same_decision(got, ref, "signed")
