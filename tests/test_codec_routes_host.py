"""The storage-code kernels' shapes and inputs, checked without a GPU: every shape of tests/codec_cases.py reaches the kernel and
variant it names (ops.codec_route: the launchers' own decision code, nothing launched), the shapes between them reach every
variant, the inputs hold the values at which the encode arithmetic changes case, and a kernel that were wrong in one of four
plausible ways would differ from the oracle on a planted element."""
import os

import numpy as np
import pytest

import codec_cases as cc
import epilogue_cases as ec
import oracle


@pytest.fixture(scope="module")
def ops():
    from fp8q import ops as o
    return o


@pytest.fixture(scope="module")
def shapes(ops):
    return cc.build_shapes(ops)


_cache = {}


def _case(key):
    """(case, oracle codes) of a key's input: shared by both directions and all phases, never modified"""
    ck = (key[1], key[2], key[3], key[6])
    if ck not in _cache:
        case = cc.case_input(key)
        _cache[ck] = (case, oracle.c_encode(case["x"], case["maxval"], *key[3]))
    return _cache[ck]


def _inputs(shapes):
    """one key per distinct input"""
    seen = {}
    for key in shapes:
        seen.setdefault((key[1], key[2], key[3], key[6]), key)
    return list(seen.values())


def test_no_tuning_variable_is_set():
    """routes are reached by shape only: the expectations hold for the launchers' defaults"""
    assert [v for v in ("FP8Q_NT_MB", "FP8Q_DIRECT_MAX_INNER") if v in os.environ] == []


def test_every_shape_reaches_its_route(ops, shapes):
    bad = []
    for key, want in shapes.items():
        got = cc.route_of(ops, key)
        if any(got[k] != v for k, v in want.items()) or got["nontemporal"]:
            bad.append((key, want, got))
    assert not bad, bad[:5]
    assert len(shapes) < 120
    big = {k[1:3] for k in shapes if k[1] * k[2] > cc.BIG}
    assert len(big) <= 2 and all(k[1] * k[2] * 4 < (64 << 20) for k in shapes), big
    assert all(len({k[3] for k in shapes if k[1:3] == b}) == 1 for b in big)        # the large shapes run one format each
    assert {k[3] for k in shapes} == set(cc.FORMATS)


def test_the_shapes_reach_every_kernel_and_variant(ops, shapes):
    reached = {}
    for key in shapes:
        r = cc.route_of(ops, key)
        for v in cc.variant(key, r):
            reached.setdefault((key[0], r["kernel"], v), []).append(key)
    want = cc.variants()
    assert want - set(reached) == set(), sorted(want - set(reached))
    assert set(reached) - want == set(), sorted(set(reached) - want)
    assert {k for _, k, _ in reached} == set(ops.CODEC_KERNELS)
    # the second grid-stride step holds whole groups in both directions, not a tail alone
    C, inner = cc.STEPS2
    assert (inner >> 4) > 256 and (inner >> 2) > 1024 and cc.route_of(ops, cc._k(True, C, inner))["grid_x"] == 1


def test_both_directions_take_the_same_route(ops, shapes):
    for key in shapes:
        a, b = cc.route_of(ops, key), cc.route_of(ops, (not key[0],) + key[1:])
        assert (not key[0],) + key[1:] in shapes, key
        assert {k: v for k, v in a.items() if k != "wide"} == {k: v for k, v in b.items() if k != "wide"}, key
        dec = b if key[0] else a
        assert not dec["wide"]


def test_route_query_errors_and_thresholds(ops):
    from fp8q._lib import CodecRouteInfo, Fp8qError, lib
    import ctypes
    with pytest.raises(Fp8qError, match="unsupported"):
        ops.codec_route(True, 2, 64, n_bits=9)
    with pytest.raises(Fp8qError, match="unsupported"):
        ops.codec_route(False, 2, 64, mbits=7)                       # no exponent bit
    with pytest.raises(Fp8qError, match="unsupported"):
        ops.codec_route(True, 0, 64, mbits=7)                        # the format is judged before the empty shape
    with pytest.raises(Fp8qError, match="invalid"):
        ops.codec_route(True, -1, 64)
    with pytest.raises(Fp8qError, match="invalid"):
        ops.codec_route(True, 2, 64, fp_mod16=2)
    with pytest.raises(Fp8qError, match="invalid"):
        ops.codec_route(True, 2, 64, code_mod16=16)
    with pytest.raises(Fp8qError, match="invalid"):
        ops.codec_route(True, 2, 64, sign_bits=2)
    info = CodecRouteInfo()
    info.kernel = 77
    assert lib().fp8q_codec_route(1, 4, 64, 3, 2.0, 8, 1, 0, 0, ctypes.byref(info)) == -1      # n_maxval neither 1 nor C
    assert lib().fp8q_codec_route(1, 4, 64, 4, 2.0, 9, 1, 0, 0, ctypes.byref(info)) == -2
    assert info.kernel == 77                                          # written on FP8Q_OK only
    assert lib().fp8q_codec_route(1, 4, 64, 4, 2.0, 8, 1, 0, 0, None) == -1
    for enc in (True, False):
        for C, inner in ((0, 64), (5, 0)):
            r = ops.codec_route(enc, C, inner)
            assert r["kernel"] is None and r["launches"] == 0
    # thresholds by arithmetic alone: the 64 MiB instance, the slabs of 65535 rows, the row length the flat kernel stops at
    assert ops.codec_route(True, 1 << 12, 4096)["nontemporal"] and not ops.codec_route(True, (1 << 12) - 1, 4096)["nontemporal"]
    assert ops.codec_route(True, 1 << 17, 147)["nontemporal"] and ops.codec_route(True, 1 << 17, 147)["kernel"] == "k_rows_flat"
    r = ops.codec_route(False, 2 * cc.SLAB + 1, 3)
    assert (r["kernel"], r["launches"], r["grid_y"]) == ("k_codec_rows", 3, cc.SLAB)
    assert ops.codec_route(True, cc.SLAB, 3)["launches"] == 1
    assert ops.codec_route(True, 3, 2047)["kernel"] == "k_rows_flat" and ops.codec_route(True, 3, 2048)["kernel"] == "k_codec_rows"
    assert ops.codec_route(True, 700, 8229)["steps"] == 2 and ops.codec_route(True, 682, 8229)["steps"] == 1
    # per tensor: one row of C * inner elements whatever the row length
    assert ops.codec_route(True, 120, 147, per_channel=False) == ops.codec_route(True, 1, 120 * 147, per_channel=False)
    assert ops.codec_route(True, 120, 147, per_channel=False)["kernel"] == "k_codec_rows"
    # one copy of the rules: the launchers hold them, the query and the entries run the same function
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fp8-quantization_amd", "csrc")
    codec = open(os.path.join(src, "fp8q_codec.hip")).read()
    assert codec.count("codec_plan(") == 4 and "2048" not in codec and "flat_nch" not in codec
    assert open(os.path.join(src, "fp8q_rows.hip")).read().count("flat_nch(") == 3      # its definition, K1's call, the codec's call


def _content(key, case, codes):
    """which of the values the encode arithmetic has cases for the input holds, from the oracle's codes and from x"""
    fmt = key[3]
    M, E = ec.fmt_me(fmt)
    x = case["x"]
    sign, ex, fr = cc.code_fields(codes, fmt)
    mv = np.broadcast_to(np.asarray(case["maxval"], np.float32).reshape(-1, 1), x.shape) if key[6] else np.full(x.shape, case["maxval"][0], np.float32)
    with np.errstate(invalid="ignore"):
        plain = np.isfinite(mv) & (mv > 0)
        val = np.abs(oracle.c_decode(codes, case["maxval"], *fmt))
        carry = plain & np.isfinite(x) & (fr == 0) & (ex >= 2) & (np.abs(x) < val)      # rounded up into the next exponent code
    sub = plain & (ex == 0) & (fr != 0)                                                  # ri < 2^M, not zero
    normal = plain & (ex >= 1) & (fr != 0)
    planted = np.zeros(x.size, bool)
    planted[case["pos"]] = True
    planted = planted.reshape(x.shape)
    # an exact tie of the default range in each binade of epilogue_cases.binades, in a row of that range; the carry right after
    # the binade's last tie k = 2^(M+1) - 1
    rows = cc.default_rows(case)
    dflt = float(case["ranges"][0])
    xb = x[rows].view(np.int32) if key[6] else x.view(np.int32)
    tie_binades, carry_tie = set(), False
    for p, k, t, s in ec.ties(fmt[0], dflt, fmt[2], fmt[1]):
        step = 2.0 ** np.rint(np.log2(s))
        if float(t) != (k + 0.5) * step or float(t) > dflt:
            continue
        if (xb == np.float32(t).view(np.int32)).any():
            tie_binades.add(p)
            if k == 2 ** (M + 1) - 1:
                hit = (x.view(np.int32) == np.float32(t).view(np.int32)) & carry
                carry_tie |= bool(hit.any())
    return dict(sub=bool((sub & planted).any()), carry=bool((carry & planted).any()), normal=bool((normal & planted).any()),
                carry_tie=carry_tie, nan=bool(np.isnan(x).any()), inf=bool(np.isinf(x).any()),
                negzero=bool(((x == 0) & np.signbit(x)).any()), ties=tie_binades,
                masks=dict(sub=sub, carry=carry, planted=planted))


def _full(key, c):
    M, E = ec.fmt_me(key[3])
    # (the binade pmax has its last tie above maxval and the one below it at most: every binade below it must show one)
    need = {p for p in ec.binades(E) if p < (1 << E)}
    # (one exponent bit: the codes 0 and 1 share the scale of binade 1, whose carry would lie above maxval -- there is none)
    if E >= 2 and not (c["carry"] and c["carry_tie"]):
        return False
    return c["sub"] and c["normal"] and c["nan"] and c["inf"] and c["negzero"] and need <= c["ties"]


def test_the_inputs_hold_what_the_encode_arithmetic_has_cases_for(ops, shapes):
    """per case: the planted edge values are in x bit for bit, the oracle encodes and decodes it, every code is below 2^n_bits.
    The three cases of the field (p << M) + |r| - 2^M -- subnormal, normal, carry into the next exponent code --, a NaN, an
    infinity, a -0 and an exact tie in every binade are in every case that has room for the edge list, and in at least one case of
    every (direction, kernel, variant)."""
    full = {}
    for key in _inputs(shapes):
        case, codes = _case(key)
        fmt = key[3]
        x = case["x"].reshape(-1)
        assert np.array_equal(x[case["pos"]].view(np.int32), case["val"].view(np.int32)), key
        assert codes.dtype == np.uint8 and int(codes.max()) < (1 << fmt[1]), key
        back = oracle.c_decode(codes, case["maxval"], *fmt)
        assert back.shape == case["x"].shape
        c = _content(key, case, codes)
        full[(key[1], key[2], key[3], key[6])] = _full(key, c)
        if cc.is_rich(key, case):
            assert _full(key, c), (key, {k: v for k, v in c.items() if k != "masks"})
        if not key[6] and key[2] >= 4096:
            assert _full(key, c), (key, {k: v for k, v in c.items() if k != "masks"})
    assert sum(full.values()) >= 20
    seen = set()
    for key in shapes:
        if full[(key[1], key[2], key[3], key[6])]:
            seen |= {(key[0], cc.route_of(ops, key)["kernel"], v) for v in cc.variant(key, cc.route_of(ops, key))}
    assert cc.variants() - seen == set(), sorted(cc.variants() - seen)
    assert {k[3] for k in shapes if full[(k[1], k[2], k[3], k[6])]} == set(cc.FORMATS)


def test_edge_values_lie_on_both_sides_of_every_border(shapes):
    for key in _inputs(shapes):
        C, inner, fmt = key[1:4]
        case, _ = _case(key)
        placed = np.zeros(C * inner, bool)
        placed[case["pos"]] = True
        n = min(inner, ec.cycle(cc.n_edges(fmt)))
        rows = placed.reshape(C, inner)
        assert rows[:, :(n + 1) // 2].all() and rows[:, inner - (n - (n + 1) // 2):].all(), key      # both sides of every row border
        for b in range(cc.rc.CHUNK, C * inner, cc.rc.CHUNK):
            assert placed[max(b - cc.rc.BORDER, 0):b + cc.rc.BORDER].all(), (key, b)
        if C > cc.SLAB:                                                   # and of the launch border
            assert rows[cc.SLAB - 2:cc.SLAB + 2].all(), key
            assert len({case["ranges"][r] for r in range(cc.SLAB - 2, cc.SLAB + 2)}) == 4
        if key[6] and C > 1:                                              # neighbouring rows: different ranges
            assert all(repr(case["ranges"][r]) != repr(case["ranges"][r + 1]) for r in range(min(C, 40) - 1)), key


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_all_codes_holds_every_code_in_every_row(fmt):
    C = 9
    a = cc.all_codes(fmt, C)
    n = 1 << fmt[1]
    assert a.shape == (C, 3 * n) and a.dtype == np.uint8 and int(a.max()) == n - 1
    for r in range(C):
        assert np.array_equal(np.bincount(a[r], minlength=n), np.full(n, 3)) and a[r, 0] == r % n
    assert 4096 % a.shape[1] != 0
    assert cc.all_codes(fmt, 64).size > 4096 or fmt[1] < 8
    R = ec.ranges(fmt)
    y = oracle.c_decode(a, [R[r % len(R)] for r in range(C)], *fmt)
    assert y.shape == a.shape
    # codes the encoder never emits are among them: above the top code of the range, and every subnormal
    M, E = ec.fmt_me(fmt)
    top = int(oracle.c_encode(np.array([[np.inf]], np.float32), [R[0]], *fmt)[0, 0])
    sign, ex, fr = cc.code_fields(a[0], fmt)
    assert ((ex == 0) & (fr != 0)).sum() == 3 * ((1 << M) - 1) * (1 + fmt[2])
    assert top == (((1 << E) - 1) << M | ((1 << M) - 1)) or (a[0] > top).any()


# ---------------------------------------------------------------------------------------------------------------------------
# a deliberately wrong kernel would be caught: each mutation of the oracle's codes differs from them on a planted element
# ---------------------------------------------------------------------------------------------------------------------------
def _mut_sign_at_bit7(codes, fmt):
    """the sign bit at position 7 whatever n_bits is"""
    sign, _, _ = cc.code_fields(codes, fmt)
    mag = codes.astype(np.int64) & ((1 << (fmt[1] - fmt[2])) - 1)
    return (mag | (sign << 7)).astype(np.uint8)


def _mut_carry_keeps_the_exponent(codes, fmt, carry):
    """ri == 2^(M+1) encoded as (p, 0) instead of (p + 1, 0)"""
    M, _ = ec.fmt_me(fmt)
    return np.where(carry, codes.astype(np.int64) - (1 << M), codes).astype(np.uint8)


def _mut_subnormal_as_normal(codes, fmt, sub):
    """ri < 2^M encoded with exponent code 1"""
    M, _ = ec.fmt_me(fmt)
    return np.where(sub, codes.astype(np.int64) | (1 << M), codes).astype(np.uint8)


def _mut_straddle_takes_the_previous_row(key, case, codes):
    """elements b..3 of a 16-byte group that straddles a row border encoded with the previous row's range"""
    C, inner, fmt = key[1:4]
    start = np.arange(1, C, dtype=np.int64) * inner
    left = (4 - start % 4) % 4                                # elements of the new row inside the straddling group
    pos = np.concatenate([start[left > j] + j for j in range(3)])
    prev = pos // inner - 1
    out = codes.reshape(-1).copy()
    x = case["x"].reshape(-1)
    out[pos] = oracle.c_encode(x[pos][:, None], case["maxval"][prev], *fmt)[:, 0]
    return out.reshape(codes.shape), pos


def test_a_wrong_kernel_would_differ_on_a_planted_element(ops, shapes):
    caught = {"sign": [], "carry": [], "subnormal": [], "straddle": []}
    for key in _inputs(shapes):
        if key[1] * key[2] > cc.BIG:
            continue
        case, codes = _case(key)
        fmt = key[3]
        c = _content(key, case, codes)
        planted = c["masks"]["planted"]
        if fmt[2] == 1 and fmt[1] < 8 and ((_mut_sign_at_bit7(codes, fmt) != codes) & planted).any():
            caught["sign"].append(key)
        if ((_mut_carry_keeps_the_exponent(codes, fmt, c["masks"]["carry"]) != codes) & planted).any():
            caught["carry"].append(key)
        if ((_mut_subnormal_as_normal(codes, fmt, c["masks"]["sub"]) != codes) & planted).any():
            caught["subnormal"].append(key)
        if key[6] and key[2] >= 4 and key[2] % 4 and cc.route_of(ops, key)["kernel"] == "k_rows_flat":
            mut, pos = _mut_straddle_takes_the_previous_row(key, case, codes)
            diff = (mut != codes) & planted
            if diff.any():
                caught["straddle"].append(key)
                # every count of elements left in the row before, among the flat cases
                caught.setdefault("b", set()).update((np.flatnonzero(diff.reshape(-1)) // key[2] * key[2] % 4).tolist())
    assert {k[3] for k in caught["sign"]} == {(2, 4, 1), (1, 3, 1)}, caught["sign"]
    assert {k[3] for k in caught["carry"]} == {f for f in cc.FORMATS if ec.fmt_me(f)[1] >= 2}      # (one exponent bit: no carry exists)
    assert {k[3] for k in caught["subnormal"]} == set(cc.FORMATS)
    assert {k[3] for k in caught["straddle"]} >= {cc.E5M2, cc.E4M3, cc.E7, (2, 4, 1), (3, 6, 0), (1, 3, 1), (6, 8, 1)}, caught["straddle"]
    assert caught["b"] == {1, 2, 3}
    # the flat cases whose rows straddle groups are all caught, the 147-element ones included
    flat = [k for k in _inputs(shapes) if k[6] and k[2] % 4 and k[1] * k[2] <= cc.BIG and cc.route_of(ops, k)["kernel"] == "k_rows_flat"]
    assert set(flat) == set(caught["straddle"]), set(flat) - set(caught["straddle"])
