"""The row kernels' shapes and inputs, checked without a GPU: every shape of tests/rows_cases.py reaches the kernel and variant it
names (ops.rows_route: the launchers' own decision code, nothing launched), the shapes between them reach every kernel and every
launcher-chosen variant, and the inputs hold the hand-picked hard values where the kernels take their special paths."""
import os

import numpy as np
import pytest

import epilogue_cases as ec
import oracle
import rows_cases as rc

# every tuning variable the row launchers read (csrc/fp8q_quant.hip, fp8q_rows.hip, fp8q_rowsreg.hip, fp8q_minmax.hip, fp8q_common.h)
TUNING = ["FP8Q_NT_MB", "FP8Q_K1_BLOCKS", "FP8Q_K1_SMALL_M", "FP8Q_DIRECT_MAX_INNER", "FP8Q_FLAT", "FP8Q_FLAT_LDS_KB", "FP8Q_FLAT_NCH",
          "FP8Q_STAGED", "FP8Q_STAGED_GRID", "FP8Q_FLAT_GRID", "FP8Q_STAGED_MM_GRID", "FP8Q_DIRECT_ELEMS", "FP8Q_K2_PASSES",
          "FP8Q_DIRECT_LDS_KB", "FP8Q_K2_BLOCKS", "FP8Q_SMALL_FUSED", "FP8Q_FUSED_REG", "FP8Q_K3_BLOCKS"]


@pytest.fixture(scope="module")
def ops():
    from fp8q import ops as o
    return o


@pytest.fixture(scope="module")
def shapes(ops):
    return rc.build_shapes(ops)


def test_no_tuning_variable_is_set():
    """routes are reached by shape only: the expectations below hold for the launchers' defaults"""
    assert [v for v in TUNING if v in os.environ] == []
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fp8-quantization_amd", "csrc")
    import re
    read = set()
    for unit in ("fp8q_quant.hip", "fp8q_rows.hip", "fp8q_rowsreg.hip", "fp8q_minmax.hip"):
        read |= set(re.findall(r'"(FP8Q_[A-Z0-9_]+)"', open(os.path.join(src, unit)).read()))
    # (the others are not launch geometry: the workspace check, the reducer's spin limit, the selection kernel's own cap)
    assert read - {"FP8Q_DEBUG_WS", "FP8Q_SEL_CAP"} <= set(TUNING), sorted(read - set(TUNING))


def test_every_shape_reaches_its_route(ops, shapes):
    bad = []
    for key, want in shapes.items():
        got = rc.route_of(ops, key)
        if any(got[k] != v for k, v in want.items()) or got["launches"] != 1 or got["nontemporal"]:
            bad.append((key, want, got))
    assert not bad, bad[:5]
    assert len(shapes) < 160
    big = [k for k in shapes if k[1] * k[2] > (1 << 20)]
    assert len(big) <= 3 and all(k[1] * k[2] * 4 < (64 << 20) for k in shapes), big


def test_the_shapes_reach_every_kernel_and_variant(ops, shapes):
    reached = {}
    for key in shapes:
        r = rc.route_of(ops, key)
        reached.setdefault((key[0], r["kernel"], rc.variant(key, r)), []).append(key)
    want = rc.variants()
    # k_rows_reg's instances: the pinned list is what the query finds over every multiple of 4 in 128..8192
    assert sorted(rc.reg_sweep(ops)) == sorted(rc.REG_PAIRS)
    assert want - set(reached) == set(), sorted(want - set(reached))
    assert set(reached) - want == set(), sorted(set(reached) - want)
    assert {k for _, k, _ in reached} == set(ops.ROWS_KERNELS)
    # the resident grid of k_rows_flat: more tiles than its 1024 blocks
    res = [k for k in shapes if k[0] == "quantize" and rc.route_of(ops, k)["kernel"] == "k_rows_flat" and rc.route_of(ops, k)["grid_x"] == 1024]
    assert len(res) == 1 and -(-(res[0][1] * res[0][2] // 4) // 1024) > 1024 * rc.route_of(ops, res[0])["nch"]
    # in-place twins wherever the entry allows them
    for op in ("quantize", "minmax_quantize"):
        assert {rc.route_of(ops, k)["kernel"] for k in shapes if k[0] == op and k[6]} >= {"k_rows_direct"}


def test_route_query_errors_and_thresholds(ops):
    from fp8q._lib import Fp8qError
    with pytest.raises(Fp8qError, match="longer"):
        ops.rows_route("minmax_quantize", 2, ops.fused_max_inner() + 1)
    with pytest.raises(Fp8qError, match="unsupported"):
        ops.rows_route("quantize", 2, 64, True, 0, 16, 1)
    with pytest.raises(Fp8qError, match="invalid"):
        ops.rows_route("minmax_quantize", 2, 64, x_mod16=2)
    with pytest.raises(Fp8qError, match="invalid"):
        ops.rows_route("minmax", 0, 64)
    assert ops.rows_route("quantize", 0, 64)["kernel"] is None and ops.rows_route("quantize", 0, 64)["launches"] == 0
    # the 64 MiB threshold and the slabs of 65535 rows, by arithmetic alone
    assert ops.rows_route("quantize", 1 << 12, 4096)["nontemporal"] and not ops.rows_route("quantize", (1 << 12) - 1, 4096)["nontemporal"]
    r = ops.rows_route("quantize", 65536 + 5, 2048)
    assert (r["kernel"], r["launches"], r["grid_y"], r["nontemporal"]) == ("k_quant_rows", 2, 65535, True)
    assert ops.rows_route("minmax", 70000, 2052)["launches"] == 2
    # C * inner on either side of 16384 at one row length
    assert ops.rows_route("minmax_quantize", 64, 256)["kernel"] == "k_small_rows_fused"
    assert ops.rows_route("minmax_quantize", 65, 256)["kernel"] == "k_rows_reg"


def _placement(case, C, inner):
    pos, idx, val = case["pos"], case["idx"], case["val"]
    x = case["x"].reshape(-1)
    assert np.array_equal(x[pos].view(np.int32), val.view(np.int32))
    return pos, idx


@pytest.mark.parametrize("fmt", ec.FORMATS)
def test_quantize_inputs_hold_every_edge_value_at_every_phase_and_border(fmt):
    """on a tensor of many short rows: every edge value of every range of the format, at the four phases of a 16-byte group, in the
    first and in the last elements of a row, and on both sides of a chunk border"""
    C, inner = 1200, 147
    case = rc.case_input((C, inner), fmt, "quantize")
    pos, idx = _placement(case, C, inner)
    n_edges = len(ec.edge_values(fmt[0], 1.0, fmt[2], fmt[1]))
    R = ec.ranges(fmt)
    rng_of = (pos // inner) % len(R)
    col = pos % inner
    for k in range(len(R)):
        sel = rng_of == k
        seen = np.zeros((n_edges, 4), bool)
        seen[idx[sel], pos[sel] % 4] = True
        assert seen.all(), (fmt, R[k], np.argwhere(~seen)[:4])
        head, tail = np.zeros(n_edges, bool), np.zeros(n_edges, bool)
        head[idx[sel & (col < inner // 2)]] = True
        tail[idx[sel & (col >= inner // 2)]] = True
        assert head.all() and tail.all(), (fmt, R[k])
    assert np.array_equal(case["maxval"].view(np.int32), np.array(case["ranges"], np.float32).view(np.int32))
    # the elements around every chunk border are edge values of their rows
    placed = np.zeros(C * inner, bool)
    placed[pos] = True
    for b in range(rc.CHUNK, C * inner, rc.CHUNK):
        assert placed[b - rc.BORDER:b + rc.BORDER].all(), b
    before, after = np.zeros(n_edges, bool), np.zeros(n_edges, bool)
    before[idx[(pos % rc.CHUNK) >= rc.CHUNK - rc.BORDER]] = True
    after[idx[(pos % rc.CHUNK) < rc.BORDER]] = True
    assert before.all() and after.all()


def test_every_case_places_its_values_on_both_sides_of_its_borders(ops, shapes):
    for key in shapes:
        op, C, inner, fmt = key[:4]
        if C * inner > (1 << 20):
            continue
        case = rc.case_input((C, inner), fmt, op)
        pos, idx = _placement(case, C, inner)
        placed = np.zeros(C * inner, bool)
        placed[pos] = True
        if rc.base_op(op) == "quantize":
            n = min(inner, ec.cycle(len(ec.edge_values(fmt[0], 1.0, fmt[2], fmt[1]))))
            rows = placed.reshape(C, inner)
            assert rows[:, :(n + 1) // 2].all() and rows[:, inner - (n - (n + 1) // 2):].all(), key      # both sides of every row border
            for b in range(rc.CHUNK, C * inner, rc.CHUNK):
                assert placed[max(b - rc.BORDER, 0):b + rc.BORDER].all(), (key, b)
        else:
            # the row's own abs-max is the planted range
            mn, mx = oracle.c_minmax(case["x"], True)
            mv = oracle.c_absmax(mn, mx)
            for r, (kind, s) in enumerate(case["kinds"]):
                if kind in ("plain", "positive", "negative"):
                    assert mv[r] == np.float32(s), (key, r, kind)
                    assert abs(case["x"][r, case["planted"][r]]) == np.float32(s)
                elif kind == "nan":
                    assert np.isnan(mv[r])
                elif kind in ("+inf", "-inf"):
                    assert np.isinf(mv[r])
                elif kind in ("+0", "-0", "mixed0"):
                    assert mv[r] == 0
            if rc.base_op(op) == "minmax":      # a reference that is finite: per tensor in both batches, per channel in its finite rows
                for seed in (0, 1):
                    xb = rc.case_input((C, inner), fmt, op, seed)
                    bmn, bmx = oracle.c_minmax(xb["x"], rc.pc_of(op))
                    fin = [r for r, (kind, _) in enumerate(xb["kinds"]) if kind not in ("nan", "+inf", "-inf")] if rc.pc_of(op) else [0]
                    assert fin and np.isfinite(bmn[fin]).all() and np.isfinite(bmx[fin]).all(), (key, seed)
                if not rc.pc_of(op):
                    assert np.isnan(oracle.c_minmax(rc.case_input((C, inner), fmt, op, 0, nan=True)["x"], False)[0]).all()
            # every plain row holds eligible edge values of its own range in its first and last elements (up to the planted extreme)
            rows = placed.reshape(C, inner)
            for r, (kind, rng_r) in enumerate(case["kinds"]):
                # (a short row holds a short window of the list, which may lie wholly above a small range: test_fused_inputs_...
                #  shows that the rows of a range hold every eligible value between them)
                if kind == "plain" and inner >= 128:
                    assert rows[r, :inner // 2].sum() >= 2 and rows[r, inner // 2:].sum() >= 2, (key, r)


def _eligible(fmt, rng_r):
    ev = ec.edge_values(fmt[0], rng_r, fmt[2], fmt[1])
    with np.errstate(invalid="ignore"):
        return np.isfinite(ev) & (np.abs(ev) <= np.float32(rng_r))


@pytest.mark.parametrize("fmt", ec.FORMATS)
def test_fused_inputs_hold_every_eligible_edge_value_at_every_phase_and_border(fmt):
    """on a tensor of many short rows: every finite edge value within a row's range, for every finite positive range of the
    format, at the four phases of a 16-byte group, in the first and in the last elements of a row; and every such value of the
    list on both sides of a chunk border (any range)"""
    C, inner = 6000, 147
    case = rc.case_input((C, inner), fmt, "minmax_quantize")
    pos, idx = _placement(case, C, inner)
    n_edges = len(ec.edge_values(fmt[0], 1.0, fmt[2], fmt[1]))
    row = pos // inner
    col = pos % inner
    kinds = case["kinds"]
    plain = sorted({v for k, v in kinds if k == "plain"})
    assert len(plain) >= 6
    rng_of = np.array([v if k == "plain" else -1.0 for k, v in kinds])[row]
    any_ok = np.zeros(n_edges, bool)
    for v in plain:
        ok = _eligible(fmt, v)
        any_ok |= ok
        sel = rng_of == v
        seen = np.zeros((n_edges, 4), bool)
        seen[idx[sel], pos[sel] % 4] = True
        assert seen[ok].all(), (fmt, v, np.argwhere(~seen & ok[:, None])[:4])
        head, tail = np.zeros(n_edges, bool), np.zeros(n_edges, bool)
        head[idx[sel & (col < inner // 2)]] = True
        tail[idx[sel & (col >= inner // 2)]] = True
        assert head[ok].all() and tail[ok].all(), (fmt, v)
    before, after = np.zeros(n_edges, bool), np.zeros(n_edges, bool)
    before[idx[(pos % rc.CHUNK) >= rc.CHUNK - rc.BORDER]] = True
    after[idx[(pos % rc.CHUNK) < rc.BORDER]] = True
    assert before[any_ok].all() and after[any_ok].all(), (fmt, np.flatnonzero(any_ok & ~(before & after))[:8])


@pytest.mark.parametrize("fmt", [f for f in ec.FORMATS if float(f[0]).is_integer()])
def test_planted_ties_round_to_the_even_neighbour(fmt):
    """a default range gives an integer bias: the ties (k + 1/2) s_p are exact floats and come out at 2 floor((k + 1) / 2) s_p,
    computed here without the oracle"""
    mv = ec.default_maxval(fmt)
    M, E = ec.fmt_me(fmt)
    t = [(p, k, v, s) for p, k, v, s in ec.ties(fmt[0], mv, fmt[2], fmt[1]) if 2 ** M <= k < 2 ** (M + 1) - 1 or (p == 1 and k < 2 ** M)]
    x = np.array([v for _, _, v, _ in t], np.float32)
    # (the step is a power of two: ties() forms it through a float64 logarithm, an ulp off)
    want = np.array([2 * ((k + 1) // 2) * 2.0 ** np.rint(np.log2(s)) for _, k, _, s in t], np.float64)
    ok = want <= mv
    few = 6 if E > 0 else 3         # (without exponent bits only the ties of the one binade lie below maxval)
    assert ok.sum() >= few
    got = oracle.c_quantize(x[None, :], [mv], fmt[0], fmt[1], fmt[2])[0]
    assert np.array_equal(got[ok].astype(np.float64), want[ok]), (fmt, got[ok][:6], want[ok][:6])
    # and the case input carries them into a fused row whose range is the default one
    case = rc.case_input((40, 300), fmt, "minmax_quantize")
    row0 = case["x"][0]
    held = np.isin(x[ok].view(np.int32), row0.view(np.int32))
    assert held.sum() >= few, fmt
