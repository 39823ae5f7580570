"""Every branch of the backward kernels' shared launch plan (csrc/fp8q_bwd.h: bwd_plan), INT family (csrc/fp8q_intgrad.hip):
k_igrad_rows with a strided loop, per-channel rows split over several blocks (k_igrad_final's part_a[row * nsplit + i]),
every lane-group width of k_igrad_short with its boundaries, and blocks of k_igrad_short that take a second pass.

The shapes, the plan mirror and the classes are those of test_grad_geometry.py (whose coverage test, which needs no GPU,
maps them for both families); the criteria and the checker (_check) those of test_int_grad_kernels.py: gx bit-identical to
g * m, gdelta / gzero_float within 2^-22 (2^-21 with gradient scaling) of the float64 host sum of the same fp32 terms
relative to sum |term| per row, the "grad" workspace all zero after every call.
"""
import numpy as np
import pytest
import torch

from test_grad_geometry import (BIG, LONG_SHAPES, LOOP_C, LOOP_CLASSES, LOOP_INNER, SWEEP, SWEEP_C, SWEEP_LONG, assert_classes)
from test_int_grad_kernels import CONFIGS, EPS, F32, _bits, _case, _check, _data, _dev, _grid, _workspace_is_zero

pytestmark = pytest.mark.gpu

BIG_CONFIGS = (0, 2)            # asym8, sym_signed


def _call(x, g, delta, zf, cfg, need, gs_elems=0):
    from fp8q import ops
    _, symmetric, signed, n_bits = cfg
    flag = torch.tensor([signed], dtype=torch.bool, device="cuda") if symmetric else None
    res = ops.int_quantize_backward(_dev(x), _dev(g), _dev(delta), _dev(zf), flag, n_bits, symmetric, EPS, *need, gs_elems)
    return res


def _scaled_matches(x, g, delta, zf, cfg, full, gs_elems, what):
    """gradient scaling multiplies the finished fp32 sums by the fp32 gs (csrc/fp8q_intgrad.hip: igrad_store): one exact
    product away from the unscaled call, whatever the geometry"""
    _, symmetric, signed, n_bits = cfg
    hi = _grid(n_bits, symmetric, signed)[1]
    gs = F32(1.0 / np.sqrt(float(hi) * gs_elems))
    res = _call(x, g, delta, zf, cfg, (True, True, not symmetric), gs_elems)
    assert _workspace_is_zero(res[0]), what
    assert torch.equal(_bits(res[0]), _bits(full[0])), f"{what}: gx changes with gradient scaling"
    for a, b, name in zip(res[1:], full[1:], ("gdelta", "gzero_float")):
        assert (a is None) == (b is None)
        if a is not None:
            want = (b.cpu().numpy() * gs).astype(F32)
            assert np.array_equal(a.cpu().numpy().view(np.int32), want.view(np.int32)), f"{what}: scaled {name} is not gs * {name}"


def _gx_only_matches(x, g, delta, zf, cfg, full_gx, what):
    """SUMS = false: the call that wants gx alone, bit for bit the gx of the call with everything"""
    gx, gd, gz = _call(x, g, delta, zf, cfg, (True, False, False))
    assert gd is None and gz is None
    assert torch.equal(_bits(gx), _bits(full_gx)), f"{what}: gx of the call without sums differs"


def _run(name, C, inner, pc, want, ci, gx_only=False, specials=True):
    """below BIG elements: both with and without gradient scaling through _check; from BIG on: the unscaled call through
    _check (complete host sums), the scaled one against it.  Only tensors below 1 Mi elements stay in _case's cache."""
    cfg = CONFIGS[ci]
    assert_classes(C, inner, pc, want)
    big = C * inner >= BIG
    if C * inner < 1 << 20:
        x, g, delta, zf = _case(C, inner, pc, ci)
    else:
        x, g, delta, zf = _data(C, inner, pc, cfg, 2000 + 17 * ci + C % 97 + inner % 89, specials)
    if not pc:
        x, g = x.reshape(-1), g.reshape(-1)
    what = f"{name} [{C},{inner}] {cfg[0]}"
    gs_elems = inner if pc else C * inner
    full = _check(x, g, delta, zf, cfg, what)
    if big:
        _scaled_matches(x, g, delta, zf, cfg, full, gs_elems, what + " scaled")
    else:
        _check(x, g, delta, zf, cfg, what + " scaled", gs_elems=gs_elems)
    if gx_only:
        _gx_only_matches(x, g, delta, zf, cfg, full[0], what)
    del x, g, delta, zf, full
    torch.cuda.empty_cache()


def _cis(name):
    C, inner = LONG_SHAPES[name][:2]
    return BIG_CONFIGS if C * inner >= BIG else range(len(CONFIGS))


def _long_cases(names):
    return [pytest.param(name, ci, id=f"{name}-{CONFIGS[ci][0]}") for name in names for ci in _cis(name)]


def _run_long(name, ci, gx_only=False):
    C, inner, pc, want = LONG_SHAPES[name]
    _run(name, C, inner, pc, want, ci, gx_only)


@pytest.mark.parametrize("name,ci", _long_cases(["channel_split2", "channel_split5"]))
def test_per_channel_rows_split_over_blocks(name, ci):
    """every row against its own host sum: a row that picks up its neighbour's partials fails"""
    _run_long(name, ci)


@pytest.mark.parametrize("name,ci", _long_cases(["channel_cap1", "channel_cap2"]))
def test_per_channel_rows_block_cap_binds(name, ci):
    _run_long(name, ci)


@pytest.mark.parametrize("name,ci", _long_cases(["tensor_u1_one_block", "tensor_u1_single", "tensor_u1_strided", "tensor_u4_single",
                                                 "tensor_u4_strided", "tensor_nt"]))
def test_per_tensor(name, ci):
    _run_long(name, ci, gx_only=(name == "tensor_u1_strided" and ci == 0))


@pytest.mark.parametrize("name,ci", _long_cases(["channel_nt"]))
def test_per_channel_nontemporal_split(name, ci):
    _run_long(name, ci)


@pytest.mark.parametrize("inner", list(SWEEP))
def test_short_rows_every_group_width_and_boundary(inner):
    G = SWEEP[inner]
    want = SWEEP_LONG if G is None else {f"short G={G}", "short direct one pass"}
    for ci in range(len(CONFIGS)):
        _run("short rows", SWEEP_C, inner, True, want, ci)


@pytest.mark.parametrize("ci", BIG_CONFIGS, ids=[CONFIGS[ci][0] for ci in BIG_CONFIGS])
def test_short_rows_several_passes(ci):
    """[4194604, 5]: G = 1, 8193 blocks of two passes each, the last pass with 44 live rows of 256.  Plain random rows: the
    planted values of _data would fill all five columns, and no element would clip."""
    _run("short rows, two passes", LOOP_C, LOOP_INNER, True, LOOP_CLASSES, ci, gx_only=True, specials=False)
