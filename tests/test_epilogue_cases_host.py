"""Conditions on the INPUTS of tests/test_epilogue_cases_gpu.py, checked on the CPU: the hand-picked values really reach the
quantizer, the ties really are ties, the shapes are legal and take the route the table says.  If a builder bug turned the tie
coverage into ordinary values, the GPU file would stay green and mean nothing; this file would not."""
import numpy as np
import pytest

import oracle
import epilogue_cases as ec


def fmt_id(fmt):
    return "m%g_n%d_s%d" % fmt


@pytest.mark.parametrize("fmt", ec.FORMATS, ids=fmt_id)
def test_edge_values_survive_the_epilogue(fmt):
    """Every non-NaN edge value a case holds appears BIT FOR BIT in the pre-quantizer tensor oracle.c_affine_act(x, bn, res,
    0) -- all of them, for every finite positive range, every shape, with and without the batch norm (and its residual) --
    and with ReLU the non-negative ones do.  Over the cases of a shape (epilogue_cases.starts: one for a large tensor, windows
    of the list for a small one) every edge value sits at every one of the four phases of a 16-byte group."""
    for maxval in ec.ranges(fmt):
        if not ec.is_plain(maxval):
            continue
        n_edges = len(ec.edge_values(fmt[0], maxval, fmt[2], fmt[1]))
        for shape in ec.SHAPES:
            for use_bn, use_res in ((False, False), (True, False), (True, True)):
                phases = np.zeros((n_edges, 4), bool)
                for r, start in enumerate(ec.starts(shape, n_edges)):
                    case = ec.case_input(shape, fmt, maxval, use_bn, use_res, seed=r, start=start)
                    placed = case["placed"][~np.isnan(case["placed"])]
                    for act, want in ((0, placed), (1, placed[placed >= 0])):
                        t = ec.expected_t(case, act)
                        hit = np.isin(want.view(np.int32), t.view(np.int32))
                        assert hit.all(), (fmt, maxval, shape, use_bn, use_res, act, want[~hit][:8])
                    t = ec.expected_t(case, 0).reshape(-1)[case["pos"]]        # ... and each at the position it was put
                    want = case["edges"][case["idx"]]
                    ok = ~np.isnan(want)
                    assert np.array_equal(t[ok].view(np.int32), want[ok].view(np.int32)), (fmt, maxval, shape, use_bn, use_res)
                    phases[case["idx"], case["pos"] % 4] = True
                assert phases.all(), (fmt, maxval, shape, int((~phases).sum()))


@pytest.mark.parametrize("fmt", ec.FORMATS, ids=fmt_id)
def test_the_ties_are_ties(fmt):
    """At the format's default range (integer bias) every (k + 1/2) * s_p of the edge set that lies in binade p itself --
    k >= 2^M, or any k in the lowest binade, whose step also serves everything below it -- is a rounding tie of the oracle's
    quantizer: its two float32 neighbours quantize to values exactly one grid step s_p apart, and the tie itself lands on the
    even one.  For k < 2^M in a higher binade the value lies in a lower binade, whose finer grid holds it: it quantizes to
    itself.  Values beyond maxval are clamp probes and quantize to what maxval quantizes to."""
    mbits, n_bits, sign_bits = fmt
    M, E = ec.fmt_me(fmt)
    maxval = ec.default_maxval(fmt)
    mv32 = np.float32(maxval)
    bias = ec.bias32(fmt, maxval)
    assert bias == np.rint(bias) and abs(float(bias) - ((1 << E) >> 1)) <= 4, (fmt, maxval, bias)
    q = lambda v: oracle.c_quantize(np.array(v, np.float32), np.array([maxval], np.float32), mbits, n_bits, sign_bits)
    # what the clamp leaves: maxval itself -- except without an exponent bit, where the one grid step is 2^(1 - M - bias) and
    # maxval = (2^M - 1/2) steps is itself a tie, which rounds to the even 2^M steps (the reference's arithmetic)
    top = q([mv32])[0]
    assert top == (mv32 if E >= 1 else np.float32(2 ** M) * np.float32(2.0 ** (1 - M - float(bias))))
    n_ties = 0
    for p, k, t, s in ec.ties(mbits, maxval, sign_bits, n_bits):
        lo, hi = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf))
        s32 = np.float32(s)         # (the builder's double bias is an integer up to log2's last bits: float32 drops them)
        assert np.frexp(s32)[0] == 0.5 and t == np.float32(k + 0.5) * s32, "the step is no power of two or the tie not exact"
        ql, qt, qh = q([lo, t, hi])
        if t > mv32:
            assert ql == top and qt == top and qh == top, (fmt, p, k)
        elif k >= 2 ** M or p == 1:
            assert ql == np.float32(k) * s32 and qh == np.float32(k + 1) * s32 and qh - ql == s32, (fmt, p, k, ql, qh)
            assert qt == (ql if k % 2 == 0 else qh), (fmt, p, k, qt)
            n_ties += 1
            if sign_bits:
                assert q([-t])[0] == -qt
        else:
            assert qt == t, (fmt, p, k)
    # no exponent bit: one binade of 2^M - 1/2 steps, so k = 0, 1, 2 and 2^M - 1 (maxval itself); one exponent bit: the
    # lowest binade is also the top one and its last k lies beyond maxval; otherwise its 8 and 4 per higher binade
    assert n_ties >= (4 if E == 0 else 7 if E == 1 else 12), (fmt, n_ties)


def test_every_shape_is_legal():
    for shape in ec.SHAPES:
        N, C, HW = ec.nchw(shape)
        assert (C * HW) % 4 == 0 and N * C * HW <= 1.1e6, shape


def test_routes_of_the_shape_table():
    """fp8q_affine_act_route is host arithmetic, so the table holds on a machine without a GPU too; and it reports the
    launcher's argument errors"""
    import fp8q
    ops = fp8q.ops
    for shape, by_bn in ec.SHAPES.items():
        N, C, HW = ec.nchw(shape)
        for has_bn, (kernel, direct, launches) in by_bn.items():
            r = ops.affine_act_route(N, C, HW, has_bn)
            assert (r["kernel"], r["direct"], r["launches"]) == (kernel, direct, launches), (shape, has_bn, r)
            assert r["grid_y"] == min(N, 65535) and r["grid_x"] >= 1
    assert ops.affine_act_route(5, 2, 2, True)["cpp"] == 2 and ops.affine_act_route(6, 4, 3, True)["cpp"] == 4
    big = ops.affine_act_route(64, 64, 112 * 112, True)         # 196 MiB: the nontemporal kernel, planes longer than a piece
    assert big["kernel"] == "staged_nt" and big["direct"] and big["cpp"] == 2 and big["launches"] == 1
    assert ops.affine_act_route(0, 8, 25, True) == dict(kernel=None, direct=False, cpp=8, launches=0, grid_x=0, grid_y=0)
    with pytest.raises(fp8q.Fp8qError, match="unsupported"):
        ops.affine_act_route(2, 3, 25, True)                    # C * HW = 75
    with pytest.raises(fp8q.Fp8qError, match="invalid"):
        ops.affine_act_route(2, 0, 25, True)
