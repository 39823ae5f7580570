"""The chunked kernels' shapes and inputs, checked without a GPU: every shape of tests/chunk_cases.py reaches the route fields it
names (ops.chunk_route: the launchers' own decision code, nothing launched), the shapes between them reach every value of the
completeness list, the LDS bound and the magic division hold by brute force, and a kernel that were wrong in one of five
plausible ways would differ from the oracle on a planted element."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chunk_cases as cc


@pytest.fixture(scope="module")
def ops():
    from fp8q import ops as o
    return o


def test_no_tuning_variable_is_set():
    assert [v for v in ("FP8Q_NT_MB",) if v in os.environ] == []


def test_every_shape_reaches_its_route(ops):
    bad = []
    for key, want in cc.SHAPES.items():
        got = cc.route_of(ops, key)
        if any(got[k] != v for k, v in want.items()):
            bad.append((key, want, got))
        assert key[0] * key[1] <= 50000, key
        assert got["lds_bytes"] == 16 * got["rows_per_chunk"]
        assert (got["magic"] == 0) == (key[1] == 1 or not key[2]), key
        # the half kernels: the same geometry, no VEC instance
        h = cc.route_of(ops, key, elem_bytes=2)
        assert not h["vec"] and {k: v for k, v in h.items() if k != "vec"} == {k: v for k, v in got.items() if k != "vec"}
    assert not bad, bad
    assert cc.route_of(ops, (8203, 1, True))["lds_bytes"] == 65568 and cc.route_of(ops, (4097, 1, True))["lds_bytes"] == 65552
    for C in cc.SIGN_C:
        for sym in (False, True):
            for sets in (False, True):
                r = ops.chunk_route(C, 2, symmetric=sym, sets_range=sets)
                assert r["sign_prepass"] == (sym and sets and C > cc.SIGN_INLINE), (C, sym, sets)
    for key in cc.UNALIGNED:
        for i, o in ((4, 0), (0, 4), (4, 4)):
            r = cc.route_of(ops, key, in_mod16=i, out_mod16=o)
            assert not r["vec"] and all(r[k] == v for k, v in cc.SHAPES[key].items() if k != "vec"), (key, r)


def test_the_shapes_reach_every_value_of_the_completeness_list(ops):
    reached = set()
    for key in cc.SHAPES:
        reached |= cc.completeness(key, cc.route_of(ops, key))
    for key in cc.UNALIGNED:
        reached |= cc.completeness(key, cc.route_of(ops, key, in_mod16=4))
    for C in cc.SIGN_C:
        reached |= cc.completeness((C, 2, True), ops.chunk_route(C, 2, symmetric=True, sets_range=True))
    assert reached == cc.COMPLETE, (cc.COMPLETE - reached, reached - cc.COMPLETE)


def test_the_tight_shape_by_brute_force(ops):
    C, inner, chunk = cc.TIGHT
    r = cc.route_of(ops, (C, inner, True))
    counts = [cc.chunk_rows(C, inner, b)[1] for b in range(r["grid_x"])]
    assert counts[chunk] == r["rows_per_chunk"] == 180 == cc.CHUNK // inner + 2 and max(counts) == 180
    assert chunk * cc.CHUNK % inner == inner - 1 and 4094 % inner == 0
    # one pass and two passes of the row setup
    assert [cc.chunk_rows(600, 16, b)[1] for b in range(3)] == [256, 256, 88]
    assert [cc.chunk_rows(600, 15, b)[1] for b in range(2)] == [274, 274]       # (the query's bound: 275)
    # phases 0, 1, 2 in turn
    assert [b * cc.CHUNK % 3 for b in range(3)] == [0, 1, 2] and [b * cc.CHUNK % 5 for b in range(3)] == [0, 1, 2]


def _max_overlap(inner):
    """the largest number of rows a full chunk overlaps over every phase that occurs (e0 a multiple of 4096), rows unbounded"""
    e0 = np.arange(min(inner, 8200), dtype=np.int64) * cc.CHUNK      # `inner` chunks: the phases repeat after that
    return int(((e0 + cc.CHUNK - 1) // inner - e0 // inner + 1).max())


def test_the_lds_bound_by_brute_force(ops):
    """For every row length the rows any chunk overlaps fit the query's rows_per_chunk, which is never more than two entries
    above what some chunk needs, and is met exactly by the odd divisors of 4094 above 1: a chunk begins on a row's last element
    (phase inner - 1) and ends on another row's first.  (Phases are multiples of gcd(4096, inner), so an even divisor never has
    the odd phase inner - 1, and with inner == 1 a row's last element is its first: 4096 entries are used of 4098.)"""
    tight = []
    for inner in range(1, 8201):
        C = 3 * cc.CHUNK // inner + 8200          # every phase occurs, and C does not cap the bound
        r = ops.chunk_route(C, inner)
        m = _max_overlap(inner)
        assert r["rows_per_chunk"] == cc.CHUNK // inner + 2 and r["lds_bytes"] == 16 * r["rows_per_chunk"]
        assert m <= r["rows_per_chunk"], inner
        if m == r["rows_per_chunk"]:
            tight.append(inner)
        # element by element on a few lengths, to check the closed form above
        if inner in (1, 2, 3, 23, 89, 1365, 2047, 4095, 4096, 4097):
            assert max(cc.chunk_rows(51 * cc.CHUNK // inner + 2, inner, b)[1] for b in range(min(inner, 50))) <= m
        assert m >= r["rows_per_chunk"] - 2, inner
    assert {23, 89, 2047} <= set(tight) and {i for i in range(3, 4095, 2) if 4094 % i == 0} == {23, 89, 2047}
    assert not {1, 2, 46, 178, 4094} & set(tight)
    assert _max_overlap(1) == cc.CHUNK and _max_overlap(2) == cc.CHUNK // 2
    # a C below the bound caps it
    assert ops.chunk_route(7, 3)["rows_per_chunk"] == 7 and ops.chunk_route(4097, 1)["rows_per_chunk"] == 4097


def test_magic_division_exhaustively(ops):
    for inner in range(2, 4096):
        magic = np.uint64(ops.chunk_route(5000, inner)["magic"])
        assert magic != 0
        l = np.arange(inner + cc.CHUNK, dtype=np.uint64)
        assert np.array_equal((l * magic) >> np.uint64(32), l // np.uint64(inner)), inner
    assert ops.chunk_route(5000, 1)["magic"] == 0 and ops.chunk_route(5000, 7, per_channel=False)["magic"] == 0


def test_route_query_errors(ops):
    from fp8q._lib import ChunkRouteInfo, Fp8qError, lib
    for kw in (dict(C=0, inner=4), dict(C=4, inner=0), dict(C=-1, inner=4), dict(C=4, inner=4, elem_bytes=3),
               dict(C=4, inner=4, in_mod16=16), dict(C=4, inner=4, out_mod16=-1), dict(C=2, inner=1 << 31),
               dict(C=1 << 40, inner=1 << 30)):
        with pytest.raises(Fp8qError, match="invalid"):
            ops.chunk_route(**kw)
    info = ChunkRouteInfo()
    info.grid_x = 77
    L = lib()
    assert L.fp8q_chunk_route(4, 64, 3, 4, 0, 0, 0, 0, ctypes.byref(info)) == -1          # n_range neither 1 nor C
    assert L.fp8q_chunk_route(0, 64, 1, 4, 0, 0, 0, 0, ctypes.byref(info)) == -1
    assert info.grid_x == 77                                                              # written on FP8Q_OK only
    assert L.fp8q_chunk_route(4, 64, 4, 4, 0, 0, 0, 0, None) == -1
    assert L.fp8q_chunk_route(4, 64, 4, 4, 0, 0, 0, 0, ctypes.byref(info)) == 0 and info.grid_x == 1
    # a per-tensor row may be longer than 32 bits allow a per-channel one; the nontemporal instance by arithmetic alone
    assert ops.chunk_route(2, 1 << 31, per_channel=False)["grid_x"] == 1 << 20
    assert ops.chunk_route(1 << 12, 4096)["nontemporal"] and not ops.chunk_route((1 << 12) - 1, 4096)["nontemporal"]
    assert ops.chunk_route(1 << 13, 4096, elem_bytes=2)["nontemporal"] and not ops.chunk_route(1 << 12, 4096, elem_bytes=2)["nontemporal"]
    # one copy of the rules: the launches and the query run the same functions
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fp8-quantization_amd", "csrc")
    text = {f: open(os.path.join(src, f)).read() for f in os.listdir(src) if f.endswith((".hip", ".h"))}
    assert text["fp8q_intq.h"].count("a.nc_max =") == 1 and [f for f, t in text.items() if "kIntChunk / inner" in t] == ["fp8q_intq.h"]
    assert sum(t.count("a.nc_max * sizeof(float4)") for t in text.values()) == 1
    assert sum(t.count("> kSignInline") for t in text.values()) == 1
    users = [f for f, t in text.items() if "int_plan(" in t]
    assert sorted(users) == ["fp8q_codec_h16.hip", "fp8q_int.hip", "fp8q_inth16.hip", "fp8q_intq.h"], users


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_inputs_are_planted_where_the_geometry_has_borders():
    for key in cc.SHAPES:
        C, inner, pc = key
        for case in (cc.int_case(key), cc.ocp_case(key, "e4m3fn")):
            n = case["n_edges"]
            placed = np.zeros(C * inner, bool)
            placed[case["pos"]] = True
            rows = placed.reshape(C, inner)
            m = min(inner, n)
            assert rows[:, :(m + 1) // 2].all() and rows[:, inner - (m - (m + 1) // 2):].all(), key
            for b in range(cc.CHUNK, C * inner, cc.CHUNK):
                assert placed[b - cc.BORDER:b + cc.BORDER].all(), (key, b)
            assert np.unique(case["idx"]).size == n, key                   # the whole list is in every case
            if inner < n:
                assert placed.all()
        if pc and C > 2:
            xmin, xmax = cc.int_ranges(C)
            assert xmin[1] == 0 and xmax[1] == 0 and xmin[2] > 0
            k = cc.int_consts(xmin, xmax, 8, False)
            ratio = k["scale"][1:40] / k["scale"][:min(C, 40) - 1]
            assert ((ratio >= 50) | (ratio <= 0.02)).all(), key             # neighbours: orders of magnitude apart


@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("n_bits", [2, 8, 16])
def test_the_numpy_chain_is_the_quantizer_classes_chain(sym, n_bits):
    """chunk_cases' numpy arithmetic (what the mutation check below recomputes) equals quantization/uniform.py on the CPU"""
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    for key in ((2140, 23, True), (8203, 1, True), (1, 12291, False)):
        case = cc.int_case(key, n_bits, sym)
        q = (SymmetricUniformQuantizer if sym else AsymmetricUniformQuantizer)(n_bits=n_bits, per_channel=key[2])
        q.set_quant_range(torch.from_numpy(case["xmin"]), torch.from_numpy(case["xmax"]))
        k = cc.int_consts(case["xmin"], case["xmax"], n_bits, sym)
        assert np.array_equal(q._delta.numpy().view(np.int32), k["delta"].view(np.int32))
        if not sym:
            assert np.array_equal(q._zero_float.numpy().view(np.int32), k["zf"].view(np.int32))
        else:
            assert bool(q._signed) == k["sign"]
        y = q(torch.from_numpy(case["x"])).numpy().reshape(-1)
        got = cc.int_values(case["x"], k, case["rows"])
        assert np.array_equal(np.isnan(y), np.isnan(got))
        assert np.array_equal(np.nan_to_num(y).view(np.int32), np.nan_to_num(got).view(np.int32)), key


def _ocp_codes(x, maxval, rows, fmt):
    """tests/test_ocp_gpu.py's oracle with the range entry of every element given"""
    tf = {"e4m3fn": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[fmt]
    fmax = cc.OCP_FMAX[fmt]
    scale = torch.max(torch.from_numpy(maxval), torch.tensor(cc.EPS, dtype=torch.float32)) / fmax
    q = torch.clamp(torch.from_numpy(x.reshape(-1)) / scale[torch.from_numpy(rows)], -fmax, fmax)
    return torch.where(torch.isnan(q), torch.tensor(0x7F, dtype=torch.uint8), q.to(tf).view(torch.uint8)).numpy()


def _differs_on_planted(a, b, pos):
    a, b = a[pos], b[pos]
    if a.dtype.kind == "f":
        return bool(((np.isnan(a) != np.isnan(b)) | (np.nan_to_num(a).view(np.int32) != np.nan_to_num(b).view(np.int32))).any())
    return bool((a != b).any())


def test_a_wrong_kernel_would_differ_on_a_planted_element(ops):
    """the oracle output of each per-channel case, recomputed with a wrong row index, differs from the true one on a planted
    element wherever the fault changes any row index at all"""
    caught = {"border": set(), "phase": set(), "last_entry": set()}
    for key in cc.SHAPES:
        C, inner, pc = key
        if not pc:
            continue
        nc_max = cc.route_of(ops, key)["rows_per_chunk"]
        true = cc.rows_true(C, inner)
        muts = {"border": cc.rows_border_one_low(C, inner), "phase": cc.rows_phase_zero(C, inner),
                "last_entry": cc.rows_last_entry_missing(C, inner, nc_max)}
        ic = cc.int_case(key)
        k = cc.int_consts(ic["xmin"], ic["xmax"], 8, False)
        y = cc.int_values(ic["x"], k, true)
        oc = cc.ocp_case(key, "e4m3fn")
        codes = _ocp_codes(oc["x"], oc["maxval"], true, "e4m3fn")
        for name, rows in muts.items():
            if np.array_equal(rows, true):
                continue                                   # the fault cannot show at this shape
            assert _differs_on_planted(cc.int_values(ic["x"], k, rows), y, ic["pos"]), (name, key, "int")
            assert _differs_on_planted(_ocp_codes(oc["x"], oc["maxval"], rows, "e4m3fn"), codes, oc["pos"]), (name, key, "ocp")
            caught[name].add(key)
    multi = {k for k in cc.SHAPES if k[2] and k[0] * k[1] > cc.CHUNK}
    # the row index at a border: every shape whose border falls inside a row or behind row 0
    assert caught["border"] == multi, multi - caught["border"]
    # the phase: every shape with a chunk that starts inside a row
    assert caught["phase"] == {k for k in multi if any(b * cc.CHUNK % k[1] for b in range(1, -(-k[0] * k[1] // cc.CHUNK)))}
    assert {(2800, 3, True), (1700, 5, True), (2140, 23, True), (5, 4095, True), (5, 4097, True)} <= caught["phase"]
    # the last LDS entry: used only where a chunk's row count meets rows_per_chunk -- the bound itself at the tight shape, the
    # row count C where that caps it; never with inner == 1 and more than 4096 rows (4096 entries are used of 4097 / 4098)
    full = {k for k in multi | {(4096, 1, True), (2048, 2, True)}
            if max(cc.chunk_rows(k[0], k[1], b)[1] for b in range(-(-k[0] * k[1] // cc.CHUNK))) == cc.SHAPES[k]["rows_per_chunk"]}
    assert caught["last_entry"] == full and cc.TIGHT[:2] + (True,) in full
    assert not {(4097, 1, True), (8203, 1, True), (600, 16, True), (2800, 3, True)} & full


def test_a_partial_sign_fold_would_be_seen():
    for C in cc.SIGN_C:
        seen = {1024: [], 2048: []}
        for name, (xmin, sign) in cc.sign_inputs(C).items():
            assert cc.sign_of(xmin) == sign, (C, name)
            case = cc.sign_case(C, name)
            k = cc.int_consts(case["xmin"], case["xmax"], 8, True)
            assert k["sign"] == sign
            rows = cc.rows_true(C, 2)
            y = cc.int_values(case["x"], k, rows)
            for first in seen:
                wrong = cc.sign_of(xmin, first)
                if wrong != sign:
                    y2 = cc.int_values(case["x"], cc.int_consts(case["xmin"], case["xmax"], 8, True, sign=wrong), rows)
                    assert _differs_on_planted(y2, y, np.arange(y.size)), (C, name, first)
                    seen[first].append(name)
        assert set(seen[1024]) == {"last_negative", "negative_at_1500", "nan_last"}, (C, seen)
        # (the first 2048 entries are all of them at C = 2048)
        assert set(seen[2048]) == (set() if C == 2048 else {"last_negative", "nan_last"}), (C, seen)
